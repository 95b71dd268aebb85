/* include/btlbf.h -- C ABI of the MI355X-native k-mer Bloom filter engine.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  The C++ shims
 * in include/btlbf/ (same class names and methods as the reference's public headers) and the
 * Python host code in btl_bloomfilter_amd/ are thin callers of these entry points; every entry
 * point that computes runs hand-written HIP kernels for gfx950 (btl_bloomfilter_amd/csrc/).
 * There is no CPU fallback: on a machine without a usable GPU the compute calls return
 * BTLBF_EHIP and btlbf_last_error() says why.
 *
 * The reference (bcgsc/btl_bloomfilter, /root/reference) has no FFI layer; its boundary is its
 * C++ header API.  Each entry below cites the reference interface it replaces (file:line).
 *
 * Conventions
 *  - every function returns 0 (BTLBF_OK) or a BTLBF_E* code; btlbf_last_error() (thread-local)
 *    holds a message for the last failure on the calling thread.
 *  - `mem` says where the caller's buffers live: BTLBF_HOST (pageable/pinned host memory; the
 *    library stages through its own device scratch) or BTLBF_DEVICE (HBM pointers, used as-is).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream; BTLBF_STREAM_PER_THREAD = HIP's
 *    per-thread default stream, which lets BTLBF_HOST calls of different host threads overlap).  Work on one
 *    filter is ordered by the stream; BTLBF_HOST calls synchronise before returning.
 *  - streams: a BTLBF_DEVICE call reads ALL of its inputs and writes ALL of its outputs in the order of `stream` --
 *    the sequence bytes, `starts`, ids, hash rows and raw k-mers, the probability and minimum-count tables of the
 *    classify calls and the running totals a call adds to.  Inputs that work queued earlier on that stream produces
 *    need no host synchronisation (btlbf_interleave_mates on a stream and btlbf_mibf_classify_pairs of its buffer
 *    and offsets on the same stream, with nothing in between), and work queued on the stream after the call has
 *    returned sees its outputs and its changes to the filter.  The stream may be a non-blocking one, which the
 *    NULL stream does not wait for.  Where the host has to look at an input (the miBF calls cut their batches on
 *    `starts`) or at a result (counts the call returns by value), the call waits for `stream` itself; a DEVICE
 *    call may therefore return before or after its work has run, and the caller assumes neither.  Using one filter
 *    from two streams without an event between them is the caller's race.  The calls whose results are
 *    host-visible and that take no stream wait for ALL streams of the device before they look at the array:
 *    btlbf_download, btlbf_upload, btlbf_store / btlbf_store_shard, the judges (btlbf_popcount,
 *    btlbf_filtered_popcount, btlbf_digest, btlbf_compare), the filter algebra (btlbf_clone, btlbf_combine,
 *    btlbf_fold, btlbf_threshold_bits), btlbf_rank_create, btlbf_mibf_create and
 *    btlbf_mibf_load; asynchronous DEVICE calls on any stream may precede them without a synchronisation by the
 *    caller.  tests/test_gpu_stream_order.py holds the calls to this with inputs that are still in flight on a
 *    non-blocking stream when the call is issued.
 *  - threads: every entry point that takes a filter holds the filter's internal lock for its whole duration
 *    (a filter keeps device scratch between calls), so ONE filter may be driven from many host threads -- the
 *    calls are serialised, the parallelism is inside each batch call -- and different filters run
 *    concurrently.  One exception, for the reference's per-read query loops: a read-only call on a small
 *    BTLBF_HOST buffer (btlbf_contains_hashes, btlbf_contains_seqs through the calling thread's pinned mailbox)
 *    gives the lock back as soon as its kernel is launched and only then waits for it, so such calls from
 *    different threads overlap (pass BTLBF_STREAM_PER_THREAD).  This is what makes the C++ shims safe for the reference's own threading pattern
 *    (OpenMP threads calling insert()/contains() on one filter, Tests/AdHoc/ParallelFilter.cpp:104-122;
 *    the reference itself relies on byte atomics, BloomFilter.hpp:177,191,206-210).  btlbf_destroy must not
 *    race with other calls on the same filter.  On one thread, btlbf_route_seqs may run on a second
 *    stream while btlbf_apply_routed* runs on the first (they share no scratch).
 *  - a "sequence buffer" is `len` bytes of nucleotide text.  Windows (k-mers) are identified by
 *    the byte offset p of their first base.  A window is *clean* iff all k bytes are bases the
 *    reference accepts (seedTab != 0, vendor/nthash.hpp:195-228: A C G T U, either case, and
 *    the raw bytes 1 3 4 5 7) and it does not cross a sequence boundary.  Exactly the clean
 *    windows are the k-mers ntHashIterator emits (vendor/ntHashIterator.hpp:59-86).
 *  - k-mer sizes: btlbf_create, btlbf_create_shard, btlbf_load, btlbf_hash_seqs and btlbf_hash_kmers take
 *    kmer_size 1 .. 32768 and return BTLBF_EINVAL outside; every sequence and raw-k-mer call of a filter works over
 *    that whole range (plain ntHash above k = 128 starts each lane's first window by Horner's rule instead of from
 *    a positional table).  The miBF calls take the k of their stage-1 filter; the btlbf_count_windows_* calls,
 *    which do not hash, take any k from 1 to 2^31 - 1.
 *    Spaced seeds (btlbf_set_spaced_seeds, btlbf_hash_seqs with seeds, btlbf_mibf_create over such a filter) take
 *    k <= 1024, and their tables must fit the 160 KB of LDS of a workgroup next to the tile image:
 *      floor16(2048 + k + 29) + (k + 1) * 128 + ceil16(2 * D) + ceil16(4 * U) + 1536 <= 163840
 *    with D = don't-care positions summed over the seeds and U = entries of the list of distinct don't-care
 *    offsets (kept only when it has at most 64 entries, fillers included; else 0).  Up to k = 900 every seed set
 *    fits; at k = 1024, D <= 14008 (16 seeds of weight 2 have 16352).  A seed set beyond that is refused with
 *    BTLBF_EINVAL by the call that sets it -- the message names k, the seed count and the bytes asked for and
 *    available -- before anything is allocated or launched; btlbf_plan_spaced_lds gives the same answer without a
 *    device.
 *    The partitioned pipeline (btlbf_set_insert_mode / btlbf_set_query_mode, PARTITIONED or AUTO) hashes in its
 *    pass A, whose tile image shares the LDS with the partitioning rings: plain ntHash fits up to k = 16098 with
 *    32 level-0 bins, 13410 with 256, 10338 with 512 and 4194 with 1024 bins (btlbf_plan_pass_a tells for a given
 *    k and bin count).  Above that a call in either mode is carried out by the direct kernels, with the
 *    same result; the profile (btlbf_get_profile) shows insert_direct / query_direct instead of insert_hash /
 *    query_hash.  tests/test_gpu_large_k.py holds the calls to all of this on either side of each size.
 *  - sequence boundaries inside a buffer are described by a btlbf_layout:
 *      starts != NULL : n_seqs+1 ascending byte offsets (starts[0]=0 .. starts[n_seqs]=len)
 *      else read_len>0: back-to-back reads of exactly read_len bytes (len % read_len == 0)
 *      else           : the whole buffer is one sequence
 *    `starts` lives in the same memory space as the sequence buffer.
 *  - per-window results are bitmaps of ceil(len/64) uint64_t words: bit (p & 63) of word p >> 6
 *    belongs to the window starting at byte p; windows that are not clean report 0, and so do the bits of
 *    the last word at positions >= len: every word of a bitmap is defined.
 *  - output buffers: an output array need not be initialised by the caller.  A call that returns BTLBF_OK has
 *    stored every byte of every output it was given -- the zeros of unclean windows, of the windows past a
 *    sequence's last k-mer and of the unused records of a result row included -- and no call writes outside
 *    [out, out + size) of an output, whether the buffers are host or device memory (malloc'd or reused memory
 *    is as good as zeroed memory).  A call that returns an error may have written any part of its outputs
 *    unless its own text says that nothing is written.  Where the content of part of an output is deliberately
 *    left alone, the call's text says so (btlbf_mibf_frame_probs: frame_probs[0]); running totals that a call
 *    ADDS to (btlbf_mibf_id_counts, btlbf_mibf_classify_tally) are inputs as well and must hold the caller's
 *    values.  tests/test_gpu_output_contract.py holds the calls to this with dirty, guarded outputs.
 */
#ifndef BTLBF_H
#define BTLBF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct btlbf_filter btlbf_filter; /* opaque; owns its HBM array (BloomFilter.hpp:381,398) */

enum { BTLBF_HOST = 0, BTLBF_DEVICE = 1 };
/* BTLBF_COUNTING8 / 16 / 32 / 64: CountingBloomFilter<T> with T = uint8_t / uint16_t / uint32_t / uint64_t.  The kinds
 * wider than a byte ("wide") take the DIRECT path only: every sequence call is one fused launch on the whole filter.
 * Shards, the partitioned pipeline, the position and routing calls and btlbf_microbench return BTLBF_EINVAL for them
 * before any HIP call; each entry says so where it applies. */
enum { BTLBF_BLOOM = 0, BTLBF_COUNTING8 = 1, BTLBF_COUNTING16 = 2, BTLBF_COUNTING32 = 3, BTLBF_COUNTING64 = 4 };
enum {
	BTLBF_OK = 0,
	BTLBF_EINVAL = 1,  /* bad argument (e.g. bit count not a multiple of 8, BloomFilter.hpp:391-394) */
	BTLBF_ENOMEM = 2,
	BTLBF_EIO = 3,     /* file could not be opened/read/written (vendor/IOUtil.h:14-22) */
	BTLBF_EFORMAT = 4, /* bad magic line / missing [HeaderEnd] / missing key (BloomFilter.hpp:123-148) */
	BTLBF_EHIP = 5     /* HIP runtime error, or no GPU */
};
/* counting-filter update flavours (CountingBloomFilter.hpp:135-183) */
enum { BTLBF_INCREMENT_MIN = 0, BTLBF_INCREMENT_ALL = 1 };
/* BTLBF_ORDER_SERIAL applies k-mers one after another in buffer order on a single lane: the only
 * way incrementMin is reproducible (it is order-dependent).
 *
 * BTLBF_ORDER_PARALLEL runs one k-mer per lane.  What a call then guarantees is what EVERY interleaving of the
 * reference's per-probe atomics (CountingBloomFilter.hpp:135-183: counter loads and counter compare-and-swaps) can
 * produce, and nothing more (tests/update_order_model.py states it as checkers; tests/wide_counter_model.py restates
 * them for every width).  MAX = 2^bits - 1 is the largest value of the filter's counter: 255, 65535, 2^32 - 1, 2^64 - 1:
 *   incrementAll: exact.  Saturating +1 commutes, so the counters are those of the serial order.
 *   incrementMin, counters before -> after one call, K = clean k-mers of the call, each with its h counters:
 *     - no counter decreases, a counter at MAX stays at MAX, a counter that no k-mer of the call probes is unchanged
 *       (8-bit counters: the four counters of a 32-bit word are updated with a word compare-and-swap that never
 *       carries; 16-bit counters are updated with a 32-bit compare-and-swap on the word that holds two of them, and
 *       it never carries into the neighbour; 32- and 64-bit counters with a compare-and-swap on the counter itself);
 *     - after <= what incrementAll of the same call would give, counter by counter;
 *     - for every k-mer present: min(after[its counters]) >= min(min(before[its counters]) + 1, MAX).  One call
 *       raises the minimum of a k-mer that occurs in it by AT LEAST ONE, not by its multiplicity.  An insert is done
 *       once ONE of its compare-and-swaps m -> m + 1 has made the change (one that changed nothing reads the minimum
 *       again and retries).  With h >= 2, two concurrent inserts of one k-mer may both read the minimum m and each
 *       win the compare-and-swap on a DIFFERENT counter of the k-mer, losing it on the other's: both are done, and
 *       every counter stands at m + 1 after two occurrences -- in the reference as well.  With h = 1 there is one
 *       counter to win, so the minimum rises by the full multiplicity (up to MAX).  Callers that need
 *       "n occurrences -> minimum >= n" with h >= 2 use incrementAll or the serial order;
 *     - while no touched counter reaches MAX: |K| <= sum(after) - sum(before) <= h * |K|.
 *   insertAndCheck on a counting filter: out = 1 where the minimum before the call is >= threshold, out = 0 where
 *     the minimum in incrementAll's result is < threshold, either answer in between; the counters as incrementMin. */
enum { BTLBF_ORDER_PARALLEL = 0, BTLBF_ORDER_SERIAL = 1 };

/* hipStreamPerThread (hip_runtime_api.h), for callers that do not include the HIP headers */
#define BTLBF_STREAM_PER_THREAD ((void*)2)

typedef struct btlbf_layout {
	const uint64_t* starts; /* n_seqs+1 offsets, or NULL */
	uint64_t n_seqs;        /* used with starts */
	uint32_t read_len;      /* used when starts == NULL; 0 = one sequence */
} btlbf_layout;

const char* btlbf_last_error(void);
int btlbf_device_count(void); /* number of visible GPUs, 0 if none (never fails) */

/* ---- lifetime ------------------------------------------------------------------------------
 * BTLBF_BLOOM:     `size` = number of bits, must be a multiple of 8
 *                  (BloomFilter(size_t,unsigned,unsigned), BloomFilter.hpp:65-76,389-399)
 * BTLBF_COUNTING8: `size` = bytes requested, rounded up to a multiple of 8; one uint8_t counter
 *                  per byte (CountingBloomFilter<uint8_t>(size_t,unsigned,unsigned,unsigned),
 *                  CountingBloomFilter.hpp:31-50).  `threshold` is ignored for BTLBF_BLOOM.
 * BTLBF_COUNTING16 / 32 / 64: the same constructor for the wider T: `size` = bytes requested, rounded up to a multiple
 *                  of 8 = sizeInBytes(); btlbf_size() = sizeInBytes() / sizeof(T) counters, and positions are
 *                  hash % btlbf_size() -- the counter count, not the byte count (CountingBloomFilter.hpp:40-58).
 *                  `threshold` stays unsigned and is compared against the full-width minimum.
 * The array is allocated in the HBM of `device` and zeroed. */
int btlbf_create(btlbf_filter** out, int kind, uint64_t size, unsigned hash_num, unsigned kmer_size,
                 unsigned threshold, int device);
/* One hash-range shard of a larger filter: positions are computed modulo
 * `global_size` and this object stores [shard_index*global_size/shard_count, +global_size/shard_count).
 * Concatenating the shard bodies in index order is the single-filter body.
 * btlbf_insert_seqs on a shard sets the probes that fall inside its range and drops the others
 * (counting shards: BTLBF_INCREMENT_ALL in parallel order only); btlbf_contains_seqs answers "clean
 * window and every probe inside my range is set" (counting: "... is at least the threshold").  So W
 * shards that are each handed the same reads build the single filter's body, and the AND of their
 * answers is the single filter's contains() ("gather mode" of btl_bloomfilter_amd/sharded.py: moves
 * reads instead of probes between GPUs).  Both take the partitioned pipeline like an unsharded filter. */
/* (wide counting kinds: EINVAL -- no shards) */
int btlbf_create_shard(btlbf_filter** out, int kind, uint64_t global_size, unsigned shard_index,
                       unsigned shard_count, unsigned hash_num, unsigned kmer_size,
                       unsigned threshold, int device);
int btlbf_destroy(btlbf_filter* f); /* ~BloomFilter, BloomFilter.hpp:381 */

/* ---- BTLBloomFilter_v1 / BTLCountingBloomFilter_v1 files ------------------------------------
 * load:  BloomFilter(const string&) BloomFilter.hpp:101-116,118-166;
 *        CountingBloomFilter(const string&, unsigned) CountingBloomFilter.hpp:262-343
 * store: storeFilter BloomFilter.hpp:304-314 / CountingBloomFilter.hpp:331-342; the header bytes
 *        are those the reference writes (key order, tab indent, %#.17g doubles)
 * Counting files of every width share one magic line, and the reference writes BitsPerCounter = 8 whatever T is (the
 * member is only ever changed by loadHeader, CountingBloomFilter.hpp:109,328,357): a created filter writes 8, a loaded
 * filter echoes what its file said, and the field is not trusted for the width.  The width is the `kind` the caller
 * loads with, as T is in the reference -- which does not check that the header fits T; here a load (or
 * create_from_header) with a counting kind of width w requires BloomFilterSize * w == BloomFilterSizeInBytes and
 * otherwise returns BTLBF_EFORMAT before any HIP call, the message naming both numbers. */
int btlbf_load(btlbf_filter** out, int kind, const char* path, unsigned threshold, int device);
/* header text only (everything up to and including the "[HeaderEnd]" line) -> a zeroed filter of that geometry
 * with nEntry / Entry / dFPR taken over: what the reference's public loadHeader(std::istream&) leaves behind
 * (BloomFilter.hpp:118-166, CountingBloomFilter.hpp:84,282-343); the caller fills the body (btlbf_upload) */
int btlbf_create_from_header(btlbf_filter** out, int kind, const char* header, size_t len, unsigned threshold,
                             int device);
int btlbf_store(btlbf_filter* f, const char* path);
/* header text only (writeHeader BloomFilter.hpp:264-288, storeHeader CountingBloomFilter.hpp:344-368) */
int btlbf_header(const btlbf_filter* f, char* buf, size_t cap, size_t* len);
/* shard-aware store: shard 0 writes header+body at offset 0, shard s writes its body at
 * header_len + s*shard_bytes of the same file (SURVEY.md section 5 "Checkpoint / resume") */
int btlbf_store_shard(btlbf_filter* f, const char* path);

/* ---- attributes (getters of BloomFilter.hpp:325-327,369-379; CountingBloomFilter.hpp:78-82) -- */
int btlbf_kind(const btlbf_filter* f);
unsigned btlbf_counter_bytes(const btlbf_filter* f); /* sizeof(T): 0 for a bit filter, else 1 / 2 / 4 / 8 */
uint64_t btlbf_size(const btlbf_filter* f);        /* getFilterSize() bits / size() counters (global) */
uint64_t btlbf_size_bytes(const btlbf_filter* f);  /* sizeInBytes() (global) */
uint64_t btlbf_local_bytes(const btlbf_filter* f); /* bytes held by this object (== size_bytes unless a shard) */
unsigned btlbf_hash_num(const btlbf_filter* f);
unsigned btlbf_kmer_size(const btlbf_filter* f);
unsigned btlbf_threshold(const btlbf_filter* f);
uint64_t btlbf_get_n_entry(const btlbf_filter* f);
uint64_t btlbf_get_t_entry(const btlbf_filter* f);
void btlbf_set_n_entry(btlbf_filter* f, uint64_t v); /* setnEntry BloomFilter.hpp:373 */
void btlbf_set_t_entry(btlbf_filter* f, uint64_t v); /* settEntry BloomFilter.hpp:375 */
double btlbf_get_dfpr(const btlbf_filter* f);         /* m_dFPR: the header's dFPR field (BloomFilter.hpp:83-99,277) */
void btlbf_set_dfpr(btlbf_filter* f, double v);
void* btlbf_device_ptr(const btlbf_filter* f);       /* the HBM array (carries out a pending clear; NULL for NULL) */
int btlbf_device(const btlbf_filter* f);

/* raw array access; offset/nbytes in bytes of the local array.
   btlbf_clear is LAZY (and so is creation: a new filter is a cleared filter): it marks the array as "all zero"
   and records the point of the clear on `stream`.  If the next thing that happens is a partitioned
   btlbf_insert_seqs, its first batch builds every segment from zero in LDS and writes it out -- no memset
   sweep, no read of the old array -- and anything else that looks at the array (direct insert, queries,
   download, store, popcount, digest, compare, shard/rank/row entry points, btlbf_device_ptr) zeroes it first.
   Whichever stream carries the zeroing out first waits for the recorded point, so work queued on `stream`
   before the clear is never overtaken by it.  The one thing a lazy clear cannot serve is a raw pointer kept
   from an earlier btlbf_device_ptr call: once that function has been called on a filter, its clears are eager
   (hipMemsetAsync on `stream`). */
int btlbf_clear(btlbf_filter* f, void* stream);
int btlbf_upload(btlbf_filter* f, const void* host_src, uint64_t offset, uint64_t nbytes);
int btlbf_download(const btlbf_filter* f, void* host_dst, uint64_t offset, uint64_t nbytes);

/* How btlbf_insert_seqs applies a batch to a bit filter.  DIRECT: one atomicOr per probe (random HBM
 * access).  PARTITIONED: probe positions are radix-partitioned by filter segment and ORed into the
 * segment while it sits in LDS (streamed HBM access; needs scratch memory, pays one sweep of the
 * array per batch).  AUTO picks PARTITIONED when the batch is large relative to the filter.  The
 * filter bytes are identical either way (bit OR is order-free).  scratch_bytes caps the scratch
 * allocation (0 = up to 80 % of the free HBM).  Default: BTLBF_INSERT_AUTO, or the environment
 * variable BTLBF_INSERT_MODE=direct|partitioned.  A wide counting filter accepts AUTO and DIRECT (AUTO means direct),
 * returns EINVAL for PARTITIONED, and ignores the environment variable; the same holds for the query mode. */
enum { BTLBF_INSERT_AUTO = 0, BTLBF_INSERT_DIRECT = 1, BTLBF_INSERT_PARTITIONED = 2 };
int btlbf_set_insert_mode(btlbf_filter* f, int mode, uint64_t scratch_bytes);
/* Same choice for btlbf_contains_seqs on a bit filter.  PARTITIONED tests the partitioned positions
 * against each segment in LDS and keeps the few positions found clear; it pays off when nearly
 * every k-mer hits (a batch with many misses is redone by the direct gather kernel).  AUTO samples
 * the batch first.  Results are identical in every mode.  Environment: BTLBF_QUERY_MODE. */
int btlbf_set_query_mode(btlbf_filter* f, int mode);
/* The partitioned paths keep their scratch allocation (up to 80 % of the HBM that was free at first
 * use, or the cap given to btlbf_set_insert_mode) cached in the filter; this returns it. */
int btlbf_release_scratch(btlbf_filter* f);

/* Per-kernel timing for measurement harnesses: when on, every kernel the sequence calls launch is
 * bracketed by HIP events on the launch stream.  btlbf_get_profile synchronises those events and
 * returns accumulated milliseconds and launch counts per slot (arrays of BTLBF_PROF_SLOTS). */
enum {
	BTLBF_PROF_INSERT_DIRECT = 0, /* seq_kernel<OP_BF_INSERT>: fused ntHash + atomicOr */
	BTLBF_PROF_QUERY_DIRECT = 1,  /* seq_kernel<OP_BF_CONTAINS>: fused ntHash + gather */
	BTLBF_PROF_INSERT_HASH = 2,   /* part_hash_kernel (pass A) */
	BTLBF_PROF_INSERT_SPLIT = 3,  /* part_split_kernel (pass B) */
	BTLBF_PROF_INSERT_APPLY = 4,  /* part_apply_kernel (pass C, OR in LDS) */
	BTLBF_PROF_QUERY_HASH = 5,
	BTLBF_PROF_QUERY_SPLIT = 6,
	BTLBF_PROF_QUERY_TEST = 7,    /* part_apply_kernel<QUERY> (pass C, test in LDS) */
	BTLBF_PROF_QUERY_RESOLVE = 8, /* failed-position set + resolve pass, or direct redo of a batch */
	BTLBF_PROF_OTHER = 9,
	BTLBF_PROF_SLOTS = 10
};
int btlbf_set_profiling(btlbf_filter* f, int on);
int btlbf_get_profile(btlbf_filter* f, double* ms, unsigned* calls, int reset);

/* Use spaced-seed hashing (stHashIterator, vendor/stHashIterator.hpp:23-33,53-57) for every
 * sequence-buffer call on this filter: `seeds` are n_seeds strings of length kmer_size, '1' =
 * care; hash_num must equal n_seeds*h2.  Without this call sequences are hashed like
 * ntHashIterator (vendor/ntHashIterator.hpp:38). */
int btlbf_set_spaced_seeds(btlbf_filter* f, const char* const* seeds, unsigned n_seeds, unsigned h2);

/* ---- the hot path: hash every clean window of a sequence buffer and probe the filter --------
 * insert:   insertSeq (BloomFilterUtil.h:9-17) = ntHashIterator + BloomFilter::insert
 *           (BloomFilter.hpp:185-194); counting filters: CountingBloomFilter::insert =
 *           incrementMin (CountingBloomFilter.hpp:198-204) or incrementAll (:165-183) per `op`.
 * contains: ntHashIterator + BloomFilter::contains (BloomFilter.hpp:252-262) /
 *           CountingBloomFilter::contains (CountingBloomFilter.hpp:190-196).
 * insert_and_check: BloomFilter::insertAndCheck (BloomFilter.hpp:200-214) -- bit of window p =
 *           all h bits were already set before this window's own writes.  The windows of a call run in
 *           parallel order (one fetch-or per probe; there is no order argument), so with k-mers that share
 *           bits the answers are those of SOME interleaving of the reference's fetch-ors:
 *             - the filter afterwards is exactly what insert of the same windows gives;
 *             - a clean window whose h bits were all set before the call reports 1;
 *             - for every bit the call newly sets, at least one window that probes it reports 0 (the one whose
 *               fetch-or came first); a window with a bit that was clear and that no other window probes reports 0;
 *             - at most as many windows report 0 as bits were newly set (with h = 1: exactly as many), so a
 *               k-mer repeated in the buffer is "new" once per newly set bit at the most, never once per copy;
 *             - valid_bits = the clean windows, hit bits are 0 outside them, counts = {clean, set hit bits}.
 *           A buffer without shared bit positions gives the serial order's answers bit for bit.
 * hit_bits / valid_bits may be NULL.  counts (may be NULL) receives {clean windows, hits}; it
 * lives in `mem` space and is overwritten. */
int btlbf_insert_seqs(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                      int op, int order, int mem, void* stream);
int btlbf_contains_seqs(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                        uint64_t* hit_bits, uint64_t* valid_bits, uint64_t* counts, int mem,
                        void* stream);
int btlbf_insert_and_check_seqs(btlbf_filter* f, const char* seq, uint64_t len,
                                const btlbf_layout* layout, uint64_t* hit_bits, uint64_t* valid_bits,
                                uint64_t* counts, int mem, void* stream);
/* minCount per window (CountingBloomFilter.hpp:53-64): min_out[p] is defined for all len bytes -- the minimum for a
 * clean window, 0 for unclean windows and for the positions past a sequence's last window */
int btlbf_min_count_seqs(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                         uint8_t* min_out, uint64_t* valid_bits, int mem, void* stream);
/* The same for every counter width: min_out holds len elements of btlbf_counter_bytes(f) bytes each (uint16_t,
 * uint32_t or uint64_t for the wide kinds; BTLBF_COUNTING8: uint8_t, and the call equals the one above).  The byte
 * forms above (btlbf_min_count_seqs, btlbf_min_count_hashes) return EINVAL on a wide filter with nothing written: the
 * minimum would not fit the caller's bytes. */
int btlbf_min_count_seqs_wide(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                              void* min_out, uint64_t* valid_bits, int mem, void* stream);

/* ---- precomputed hashes: n k-mers x hash_num uint64_t, row-major ------------------------------
 * insert(const uint64_t[]) BloomFilter.hpp:185; contains(const uint64_t[]) :252;
 * insertAndCheck(const uint64_t[]) :200; CountingBloomFilter insert/incrementAll/minCount/contains */
int btlbf_insert_hashes(btlbf_filter* f, const uint64_t* hashes, uint64_t n, int op, int order,
                        int mem, void* stream);
int btlbf_contains_hashes(btlbf_filter* f, const uint64_t* hashes, uint64_t n, uint8_t* out, int mem,
                          void* stream);
int btlbf_insert_and_check_hashes(btlbf_filter* f, const uint64_t* hashes, uint64_t n, uint8_t* out,
                                  int order, int mem, void* stream);
int btlbf_min_count_hashes(btlbf_filter* f, const uint64_t* hashes, uint64_t n, uint8_t* min_out,
                           int mem, void* stream);
/* min_out: n elements of btlbf_counter_bytes(f) bytes each (see btlbf_min_count_seqs_wide) */
int btlbf_min_count_hashes_wide(btlbf_filter* f, const uint64_t* hashes, uint64_t n, void* min_out, int mem,
                                void* stream);

/* ---- raw k-mers: KmerBloomFilter::insert(const char*) / contains(const char*) --------------------
 * (KmerBloomFilter.hpp:47-74 -> NTC64(kmerSeq, k) vendor/nthash.hpp:394-439,460-465 + NTE64 :537-542)
 * `kmers` = n k-mers of kmer_size bytes each, back to back.  The values are the ones the reference's
 * x86-64 build returns on this path, which differ from the iterator's (NTMC64) for k % 4 == 0 (the table
 * walk's shift by 64, :354-356,388-391,404-406) and for k-mers with U/u (read as A, :16-86, except in a
 * one-base remainder).  Bytes that are not ACGTU/acgtu wrap the reference's uint8_t table index to some
 * other 4-mer, as there; a k-mer whose 2-/3-base remainder then indexes beyond the reference's tables has
 * no defined value and is skipped (insert: nothing, contains: 0, valid: 0).
 * op / order as btlbf_insert_hashes (counting filters); out[i] = contains() of k-mer i. */
int btlbf_insert_kmers(btlbf_filter* f, const char* kmers, uint64_t n, int op, int order, int mem,
                       void* stream);
int btlbf_contains_kmers(btlbf_filter* f, const char* kmers, uint64_t n, uint8_t* out, int mem, void* stream);
/* the hash values alone: hashes[i*hash_num ..) and (optionally) valid[i] for k-mer i; a k-mer without a defined
 * value has valid[i] = 0 and a row of zeros */
int btlbf_hash_kmers(unsigned kmer_size, unsigned hash_num, const char* kmers, uint64_t n, uint64_t* hashes,
                     uint8_t* valid, int mem, int device, void* stream);

/* ---- hash streams only (iterator parity) -------------------------------------------------------
 * ntHashIterator (vendor/ntHashIterator.hpp:38,93): hashes[p*h .. p*h+h) for window p (zeros when
 * not clean), valid_bits as above.  With seeds != NULL: stHashIterator(seq, seeds, n_seeds, h2, k)
 * (vendor/stHashIterator.hpp:53,94-103), h = n_seeds*h2 values per window and strand_bits[p] bit j =
 * strandArray()[j] (h <= 64 in that case); strand_bits[p] is 0 for windows that are not clean, all len words
 * are written.  Buffers live in `mem` space. */
int btlbf_hash_seqs(unsigned kmer_size, unsigned hash_num, const char* const* seeds, unsigned n_seeds,
                    unsigned h2, const char* seq, uint64_t len, const btlbf_layout* layout,
                    uint64_t* hashes, uint64_t* valid_bits, uint64_t* strand_bits, int mem,
                    int device, void* stream);

/* ---- statistics --------------------------------------------------------------------------------
 * getPop BloomFilter.hpp:316-323 (set bits); counting: popCount (non-zero counters) :217-228 and
 * filtered_popcount (counters >= threshold) :231-242.  Local array only for shards. */
int btlbf_popcount(btlbf_filter* f, uint64_t* out);
int btlbf_filtered_popcount(btlbf_filter* f, uint64_t* out);

/* Position-dependent digest of the local array, computed in HBM (one streaming read, like btlbf_popcount) -- what a
 * caller of the reference does with sha256sum on a stored .bf body, for arrays too large to keep two of, or to
 * download.  With w_i the i-th little-endian 64-bit word of the WHOLE filter body (zero-padded at the end) and
 * m_i = mix64(i + 1) | 1 (mix64 = the splitmix64 finaliser: z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31):
 *   out2[0] = sum over the non-zero words of w_i * m_i (mod 2^64),  out2[1] = xor over them of mix64(w_i ^ m_i).
 * A shard reports its own words with their index in the whole filter, so shard digests combine by + and ^ to the
 * digest of the unsharded filter.  Synchronises the device. */
int btlbf_digest(btlbf_filter* f, uint64_t* out2);

/* Position-wise comparison of two filters of the same kind, size (and shard range) on one device, without
 * leaving HBM -- what a caller of the reference does with two filter bodies and memcmp.  Bit filters:
 * out3 = {bits that differ, bits set only in a, bits set only in b}; counting filters: {counters that
 * differ, counters with a > b, counters with a < b}, per counter of the filter's width.  Synchronises the device. */
int btlbf_compare(btlbf_filter* a, btlbf_filter* b, uint64_t* out3);

/* ---- filter algebra: combining filters that exist ---------------------------------------------------------
 * The reference has no such operations: its users loop over getFilter() on the host (BloomFilter.hpp:373).  Here the
 * arrays stay in HBM.  The contract is exact arithmetic on positions (bits, or counters of the filter's width); since
 * positions are hash % m_size (BloomFilter.hpp:190, CountingBloomFilter.hpp:52-58) it implies three identities against
 * filters BUILT by the calls above: the union of two bit filters is the filter built from both inputs; a filter of m
 * positions folds into the filter built at m / factor; the thresholded counting filter answers contains() as the
 * counting filter does at that threshold (CountingBloomFilter.hpp:190-196).
 * All four calls are synchronous like btlbf_compare: they synchronise the device, run on the null stream and return when
 * done.  A pending btlbf_clear of an operand takes effect first.  Every refusal below is BTLBF_EINVAL before any HIP
 * call, with no filter touched, *out set to NULL (where there is one) and the reason in btlbf_last_error(). */
enum { BTLBF_COMBINE_OR = 0, BTLBF_COMBINE_AND = 1, BTLBF_COMBINE_ANDNOT = 2,   /* bit filters */
       BTLBF_COMBINE_ADD = 3, BTLBF_COMBINE_MAX = 4, BTLBF_COMBINE_MIN = 5 };   /* counting filters, every width */
#define BTLBF_COMBINE_MAX_SRCS 16

/* A second filter of the same kind, geometry, shard range, device, threshold, spaced seeds, nEntry / tEntry / dFPR and
 * BitsPerCounter echo, its body copied device to device (a cleared source gives a cleared clone, without a copy).  Insert
 * and query modes are the defaults of a new filter; scratch and profile are not copied.  Refused: a null argument. */
int btlbf_clone(btlbf_filter** out, btlbf_filter* f);

/* dst = dst OP srcs[0] OP ... OP srcs[n_srcs - 1], position by position, in ONE pass: every operand is read once and
 * dst is written once (n_srcs + 2 array lengths of traffic, where a chain of pairwise calls would move 3 n_srcs).
 *   bit filters:  OR, AND, ANDNOT (dst & ~srcs[0] & ... & ~srcs[n_srcs - 1]);
 *   counting:     ADD = min(sum, MAX) -- it saturates at the counter's maximum and never wraps, as incrementAll leaves a
 *                 counter (CountingBloomFilter.hpp:165-183) -- MAX, MIN; for counters of 8, 16, 32 and 64 bits.
 * *pop_out (may be NULL) = what btlbf_popcount(dst) would return afterwards (set bits / non-zero counters), accumulated
 * in the same pass.  dst's nEntry, tEntry, dFPR and threshold are left as they are: the library cannot know how many
 * distinct entries the result holds (the caller has btlbf_set_n_entry).  Shards of the same range combine like whole
 * filters.  All n_srcs + 1 filters are locked, in address order.
 * Refused: a null argument or handle; n_srcs == 0 or > BTLBF_COMBINE_MAX_SRCS; dst among the sources; an op that does
 * not belong to dst's kind; a source that differs from dst in kind, size, local bytes, shard range, device, hash count,
 * k-mer size or spaced seeds (both without, or the same seed strings and h2). */
int btlbf_combine(btlbf_filter* dst, btlbf_filter* const* srcs, unsigned n_srcs, int op, uint64_t* pop_out);

/* A new filter of btlbf_size(f) / factor positions whose position p combines source positions p + j * size / factor,
 * j < factor: by OR for a bit filter, by saturating ADD for a counting filter.  A bit filter built at m folds into, byte
 * for byte, the filter built at m / factor from the same data; a counting filter built with BTLBF_INCREMENT_ALL into the
 * INCREMENT_ALL filter of the smaller size.  For BTLBF_INCREMENT_MIN the folded filter is an upper bound of the smaller
 * size's filter, counter by counter, not the same filter (incrementMin looks at the counters it shares).
 * Hash count, k, spaced seeds, threshold, nEntry, tEntry and dFPR carry over; factor == 1 is btlbf_clone.
 * Refused: a null argument; a shard; factor == 0; size % factor != 0; a result the constructors could not have made
 * (above, "lifetime": size / factor bits not a multiple of 8; size / factor counters not a multiple of 8 bytes). */
int btlbf_fold(btlbf_filter** out, btlbf_filter* f, uint64_t factor);

/* From a counting filter of any width, the bit filter of btlbf_size(f) bits with bit p = (counter p >= threshold); hash
 * count, k and spaced seeds are f's, nEntry / tEntry / dFPR are 0.  threshold == 0 means f's own.  contains() of the
 * result equals CountingBloomFilter::contains at that threshold (CountingBloomFilter.hpp:190-196), k-mer for k-mer, in
 * 1/8 to 1/64 of the memory -- and the result is what btlbf_screen_seqs and btlbf_mibf_create take.
 * Refused: a null argument; a bit filter; a shard; threshold == 0 on a filter whose own threshold is 0; a counter count
 * that is not a multiple of 8 (possible for the wide kinds). */
int btlbf_threshold_bits(btlbf_filter** out, btlbf_filter* f, unsigned threshold);

/* ---- rank structure over a bit filter (miBF stage 2) ------------------------------------
 * The reference's multi-index Bloom filter maps a set bit to an index of its ID array with
 * rank(pos) = set bits before pos -- getRankPos(hash) = m_rankSupport(hash % m_bv.size()), MIBloomFilter.hpp:527,
 * and the same expression in every insert / query loop (:324,391,443,461,488,509,522) -- over
 * sdsl::bit_vector_il<512> + sdsl::rank_support_il<1> (MIBloomFilter.hpp:44,133,144,801-803; sdsl-lite is an
 * un-vendored dependency of the reference).  rank_create builds that interleaved vector in HBM from a bit
 * filter (e.g. the spaced-seed filter that is miBF stage 1, MIBFConstructSupport.hpp:75-87): record b of 9
 * uint64_t = { set bits before bit 512*b, the 8 data words of block b }.  rank_query: values are positions,
 * or hash values to be reduced modulo the filter size (values_are_hashes != 0); rank_out[i] = rank,
 * bit_out[i] = the bit itself (either may be NULL).  rank_ones = set bits in total (= entries of the ID
 * array, MIBloomFilter.hpp:573-577); rank_download copies the rank_words() interleaved words to the host. */
typedef struct btlbf_rank btlbf_rank;
int btlbf_rank_create(btlbf_rank** out, btlbf_filter* f);
void btlbf_rank_destroy(btlbf_rank* r);
uint64_t btlbf_rank_ones(const btlbf_rank* r);
uint64_t btlbf_rank_words(const btlbf_rank* r);
int btlbf_rank_download(const btlbf_rank* r, uint64_t* host_dst);
int btlbf_rank_query(const btlbf_rank* r, const uint64_t* values, uint64_t n, int values_are_hashes,
                     uint64_t* rank_out, uint8_t* bit_out, int mem, void* stream);

/* ---- multi-index Bloom filter (miBF stages 2-4: MIBloomFilter.hpp, MIBFConstructSupport.hpp) -------------
 * An ID array data[T; pop] (T = uint16_t or uint32_t: id_bytes 2 or 4) and a counter array counts[T; pop], both
 * addressed by rank(hash % size) over the rank structure above.  mask = 1 << (bits(T)-1) marks a saturated entry
 * (MIBloomFilter.hpp:36-37).  Sequences are hashed as by btlbf_hash_seqs: ntHashIterator without seeds,
 * stHashIterator(seq, seeds, h, 1, k) with seeds; only clean windows count.  ids[] holds one id per sequence of
 * the layout (uint32_t, converted to T), in the memory space `mem` of the sequence buffer.
 *  mibf_create    : MIBloomFilter(hashNum, k, bv, seeds) (MIBloomFilter.hpp:122-147) + getEmptyMIBF
 *                   (MIBFConstructSupport.hpp:92-99): rank structure, data and counts zeroed.  f must be a whole bit
 *                   filter; with spaced seeds h2 must be 1 (MIBFQuerySupport.hpp:167-168).  1..8 hash values per
 *                   window.  id_bytes other than 2 / 4: EINVAL before any HIP call.  f may be destroyed afterwards.
 *  mibf_size      : entries of the ID array (getPop, MIBloomFilter.hpp:571-578); mibf_bits: the bit vector size
 *                   (size(), :622); mibf_hash_num / mibf_kmer_size: getHashNum / getKmerSize (:531-533).
 *  mibf_set_scratch : HBM budget of one call's scratch (0 = default 2 GiB).
 *  mibf_insert_ids_seqs : insertMIBF (MIBFConstructSupport.hpp:109-130), one call per sequence s with id ids[s], in
 *                   sequence order.  Each sequence's distinct hash values are walked in ASCENDING value order (the
 *                   reference walks a dense_hash_set in an unspecified order; this rule is this library's):
 *                   r = rank(v), c = counts[r] = T(counts[r] + 1), x = T(v ^ id); setData(r, id) when c != 0 and
 *                   x % c == c - 1 (c == 0 is a wrapped counter, UB in the reference: no replacement).  setData
 *                   (MIBloomFilter.hpp:625-634) keeps the saturation bit iff the old value is > mask.  The result does
 *                   not depend on how sequences are split into calls or batches.  Needs a layout.
 *  mibf_saturate_seqs : insertSaturation -> setSatIfMissing (MIBFConstructSupport.hpp:132-214) per clean window:
 *                   seenSet and replacementIDs start with h zeros; the candidate with the LARGEST count by strict >
 *                   from 0 wins (the first maximum); mutation = setData then ++counts; fallback = saturate(hashes)
 *                   (MIBloomFilter.hpp:440-446).  order BTLBF_ORDER_SERIAL: one lane walks sequences and windows in
 *                   buffer order (the reference's loop, bit for bit).  BTLBF_ORDER_PARALLEL: every window decides
 *                   against data / counts as they stood at the start of the call; then each mutated position gets
 *                   counts += its choosers (T wrap) and the id of its last chooser in (sequence, window) order by
 *                   setData's rule against the start value; then every saturation is ORed in.  A parallel call whose
 *                   decisions do not fit the scratch budget returns ENOMEM and changes nothing.  A serial call walks
 *                   the sequences in batches under the budget; one with a sequence that does not fit alone returns
 *                   ENOMEM before any batch has run: data and counts are untouched then, too.
 *                   counts4 (optional, this memory space) = {clean windows, found, mutated, saturated}.
 *  mibf_query_seqs : getMatchSignature (MIBFQuerySupport.hpp:158-217) over atRank (MIBloomFilter.hpp:478-515):
 *                   values[len*h] (T, window p at row p): data[rank] at hit positions of a matching window, else 0;
 *                   match_bits / valid_bits: per-window bitmaps as btlbf_contains_seqs; counts2 = {clean windows,
 *                   matching windows}.  With seeds a window matches with at most max_miss clear bits; without seeds
 *                   all h bits are needed and max_miss is ignored.  (id, saturated) = (v & ~mask, v > mask).
 *  mibf_stats     : out3 = {getPop, getPopNonZero, getPopSaturated (> mask)} (MIBloomFilter.hpp:571-620).
 *  mibf_id_counts : getIDCounts (MIBloomFilter.hpp:539-551) as a device histogram: counts[n_ids] (host) +=
 *                   entries per id (v & ~mask when v > mask, else v; ids >= n_ids are not counted);
 *                   *saturated = entries > mask.
 *  mibf_download / mibf_upload / mibf_download_counts : the data / counts arrays, size * id_bytes bytes (host).
 *  mibf_store     : the data file of MIBloomFilter::store (:264-305, writeHeader :722-742), byte for byte: the packed
 *                   32-byte header {"MIBLOOMF", hlen = 32 + k*n_seeds, size, nhash, kmer, version = 1}, the seeds
 *                   (k bytes each), data little-endian.  The bit vector is NOT written (no .sdsl companion file):
 *                   store the stage-1 filter with btlbf_store.
 *  mibf_load      : MIBloomFilter(path) (:149-248): missing file EIO; wrong magic, hlen, version or a data length
 *                   other than size * id_bytes EFORMAT -- all before any HIP call.  The bit vector comes from f
 *                   (same k and hash count as the file); a popcount other than size is EFORMAT. */
typedef struct btlbf_mibf btlbf_mibf;
int btlbf_mibf_create(btlbf_mibf** out, btlbf_filter* f, unsigned id_bytes);
void btlbf_mibf_destroy(btlbf_mibf* m);
uint64_t btlbf_mibf_size(const btlbf_mibf* m);
uint64_t btlbf_mibf_bits(const btlbf_mibf* m);
unsigned btlbf_mibf_hash_num(const btlbf_mibf* m);
unsigned btlbf_mibf_kmer_size(const btlbf_mibf* m);
int btlbf_mibf_set_scratch(btlbf_mibf* m, uint64_t bytes);
int btlbf_mibf_insert_ids_seqs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                               const uint32_t* ids, int mem, void* stream);
int btlbf_mibf_saturate_seqs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                             const uint32_t* ids, int order, uint64_t* counts4, int mem, void* stream);
int btlbf_mibf_query_seqs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout, unsigned max_miss,
                          void* values, uint64_t* match_bits, uint64_t* valid_bits, uint64_t* counts2, int mem,
                          void* stream);
int btlbf_mibf_stats(btlbf_mibf* m, uint64_t* out3);
int btlbf_mibf_id_counts(btlbf_mibf* m, uint64_t* counts, uint64_t n_ids, uint64_t* saturated);
int btlbf_mibf_download(btlbf_mibf* m, void* host_dst);
int btlbf_mibf_upload(btlbf_mibf* m, const void* host_src);
int btlbf_mibf_download_counts(btlbf_mibf* m, void* host_dst);
int btlbf_mibf_store(btlbf_mibf* m, const char* path);
int btlbf_mibf_load(btlbf_mibf** out, const char* path, btlbf_filter* f, unsigned id_bytes);

/* ---- read classification over the miBF (MIBFQuerySupport.hpp) ------------------------------------------
 * mibf_classify_seqs : MIBFQuerySupport<T>::query(itr, minCount) (MIBFQuerySupport.hpp:95-109) of every sequence of the
 *   buffer, each on its own and from fresh state (init, :419-428).  A layout is required.
 *   Frames are the sequence's clean windows in position order (the valid bits of btlbf_mibf_query_seqs).  Without seeds
 *   (ntHashIterator, :408-417) a frame hits when all h bits are set; evalCount gets +1 per frame (:415) and +1 per value
 *   looked up (:437).  With seeds (stHashIterator, h2 = 1, :397-406) a frame hits with at most max_miss clear bits, only
 *   the set positions are looked up, and misses is passed on.  A hit frame runs updatesCounts (:430-518) exactly: the raw /
 *   masked seenSet rules, nonSatFrameCount and solidCount only in frames without a saturated value (solidCount only with
 *   misses == 0), both candidate rules (:495-507), updateMaxCounts with its `else if` (:522-526), and the two extraFrame
 *   statements (:509-516, extra_frame_limit < extraFrame++ with the post-increment).  The walk stops at the first frame
 *   that returns true (:102-105).  The six counters are uint16_t and wrap; satCount and evalCount are 32-bit.  Then
 *   summarizeCandiates (:555-595): the gate min_count <= best nonSatFrameCount, isValid, the sortCandidates order,
 *   isRoughlyEqualOrLarger against the first, best_hit_agree.  A sequence without a frame gives the emptyResult: 0 hits,
 *   satCount 0, evalCount 0.
 *   hits[n_seqs * max_results]: n_hits[s] is the full number of significant results of sequence s; its first
 *   min(n_hits[s], max_results) records are written in result order and the rest of its row is zero.  frameProb of a
 *   record is per_frame_prob[id].  sat_count[s] / eval_count[s] = getSatCount() / getEvalCount() after the query.
 *   hits, n_hits, sat_count, eval_count, per_frame_prob and min_count_per_id live in memory space mem.
 *   This library's rules where the reference leaves a choice:
 *   - sortCandidates is a strict order whenever two candidates' frameProb differ; full ties keep the order in which the
 *     ids first entered the candidate list.
 *   - the reference indexes m_counts, minCount and perFrameProb by id (v & ~mask when v > mask, else v itself, so an
 *     entry equal to the mask indexes as the mask); an index >= n_ids is undefined behaviour there.  Here the call first
 *     takes the largest index over the whole data array (a reduction, cached until the array next changes) and returns
 *     EINVAL with nothing written unless it is below n_ids.  Id 0 (an empty entry) is counted like any other id.
 *   - compareStdErr / compareStdErrLarger are evaluated in double with an IEEE square root and without contraction.  A
 *     reference built with contraction may fuse a - sqrt(a) * extra_count; the results agree bit for bit when
 *     extra_count is a power of two (0.5, 1, 2: the product is then exact), and only those values are pinned by tests.
 *   - candidates present but none passing isValid (the reference then reads signifResults[0] of an empty vector): 0 hits.
 *   Errors: a null pointer, max_results == 0, n_ids == 0 or n_ids > 2^(bits(T)-1): EINVAL before any HIP call.  Sequences
 *   are classified in batches under the btlbf_mibf_set_scratch budget (per base h values, a hit mask and two bitmap bits;
 *   a sequence that can meet more than 255 distinct ids also a table of its own in HBM); a single sequence that does not
 *   fit returns ENOMEM with nothing written.
 * mibf_classify_pairs : the paired overload query(itr1, itr2, minCount) (:111-130) of every read pair.  Sequences 2i and
 *   2i + 1 of the layout (starts or read_len) are mate 1 and mate 2 of pair i, as in interleaved FASTQ; n_seqs must be
 *   even (an odd count: EINVAL before any HIP call, nothing written).  The outputs have n_seqs / 2 rows.  A pair is ONE
 *   walk over the frames of both mates, into one set of counters and with one early stop, in the reference's order
 *   (:113-114): at an even frameCount the next frame of mate 1 if it has one, else of mate 2; at an odd frameCount the
 *   next frame of mate 2 if it has one, else of mate 1; frameCount counts every frame taken.  A mate's frames are its
 *   clean windows in position order, as above, and no window crosses the boundary between two mates.  Everything else --
 *   updatesCounts, evalCount, max_miss, the stop, summarizeCandiates, the rules above, max_results, mem, stream, the
 *   errors -- is the contract of mibf_classify_seqs applied to that frame sequence.  A pair without a frame in either
 *   mate gives the empty result; (s, empty) and (empty, s) give what mibf_classify_seqs gives for s.  This is neither
 *   the two mates classified alone nor the mates concatenated.  Batches are cut between pairs, never between the mates
 *   of one; the table of a pair is sized for the bytes of both mates.
 * mibf_classify_paths : out2 = {sequences walked with their table in LDS, in HBM} of the last classify call of either
 *   kind (pairs, for mibf_classify_pairs). */
typedef struct {
	uint32_t id;
	uint16_t count, nonSatCount, totalCount, totalNonSatCount, nonSatFrameCount, solidCount;
} btlbf_mibf_hit; /* 16 bytes */
typedef struct {
	double extra_count;
	uint32_t extra_frame_limit, max_miss, min_count, best_hit_agree, max_results;
} btlbf_mibf_classify_params;
int btlbf_mibf_classify_seqs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                             const btlbf_mibf_classify_params* p, const double* per_frame_prob,
                             const uint32_t* min_count_per_id, uint64_t n_ids, btlbf_mibf_hit* hits, uint32_t* n_hits,
                             uint32_t* sat_count, uint32_t* eval_count, int mem, void* stream);
int btlbf_mibf_classify_pairs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                              const btlbf_mibf_classify_params* p, const double* per_frame_prob,
                              const uint32_t* min_count_per_id, uint64_t n_ids, btlbf_mibf_hit* hits, uint32_t* n_hits,
                              uint32_t* sat_count, uint32_t* eval_count, int mem, void* stream);
int btlbf_mibf_classify_paths(btlbf_mibf* m, uint64_t* out2);

/* ---- frame probabilities and the device helpers of the file classifier ----------------------------------
 * mibf_frame_probs : MIBloomFilter<T>::calcFrameProbs(frameProbs, allowedMiss) (MIBloomFilter.hpp:664-679) over
 *   calcProbSingleFrame (:65-77), getIDCounts (:539-551) and nChoosek (:781-796); n = frameProbs.size().
 *   occupancy = getPop() / size() (set bits of the bit vector over its length); countTable = getIDCounts over n bins, from
 *   the device histogram of btlbf_mibf_id_counts; sum = countTable[1] + ... + countTable[n-1] (the reference's loop starts
 *   at 1: entries of id 0 are not counted); *sat_prop = saturated entries / sum; frame_probs[i] =
 *   calcProbSingleFrame(occupancy, h, countTable[i] / sum, allowed_miss) for 1 <= i < n.  frame_probs[0] is NOT written,
 *   as in the reference.  Host arithmetic in double in the reference's order of operations, pow from libm, without
 *   contraction (the compareStdErr rule above); nChoosek in int, as the reference computes it.
 *   Where the reference has undefined behaviour this call returns EINVAL with nothing written:
 *   - the largest id index of the data array (the cached reduction of mibf_classify_seqs) is >= n: getIDCounts would
 *     index past countTable;
 *   - allowed_miss > h: the reference's unsigned loop start h - allowed_miss wraps;
 *   - sum == 0: both divisions are by zero;
 *   - a null pointer or n == 0 (checked before any HIP call).
 * mibf_prob_single_frame : calcProbSingleFrame itself, the same arithmetic, for one frequency (no device work).
 *   allowed_misses > hash_num gives 0, as the reference's wrapped loop does.
 * interleave_mates : the interleaved buffer mibf_classify_pairs takes, built on the device from two ragged buffers
 *   (starts1 / starts2: n_pairs + 1 offsets each, starts*[0] == 0): out = mate 1 of pair 0, mate 2 of pair 0, mate 1 of
 *   pair 1, ...; out_starts[2i] = starts1[i] + starts2[i], out_starts[2i+1] = starts1[i+1] + starts2[i],
 *   out_starts[2 n_pairs] = starts1[n_pairs] + starts2[n_pairs] (2 n_pairs + 1 entries).  Any alignment of the four
 *   buffers.  mem == BTLBF_HOST: the buffers are staged.  Null pointers: EINVAL before any HIP call (seq1, seq2 and out
 *   may be null only when they hold no byte).
 * mibf_classify_tally : adds the summary of one batch of classify results (n_rows rows of max_results records) to
 *   running totals: best[id] += 1 for the id of the first record of every row with n_hits >= 1; any[id] += 1 for each of
 *   the first min(n_hits, max_results) records of every row; totals6 += {rows, rows with n_hits == 0, rows with
 *   n_hits > 1, rows with n_hits > max_results, sum of sat_count, sum of eval_count}.  best and any have n_ids entries;
 *   an id >= n_ids (classify cannot produce one) is ignored.  All arrays in memory space mem; with BTLBF_HOST they are
 *   staged and the call returns when the totals are back.  Null pointers (the four result arrays may be null when
 *   n_rows == 0), max_results == 0 or n_ids == 0: EINVAL before any HIP call. */
int btlbf_mibf_frame_probs(btlbf_mibf* m, unsigned allowed_miss, double* frame_probs, uint64_t n, double* sat_prop);
double btlbf_mibf_prob_single_frame(double occupancy, unsigned hash_num, double freq, unsigned allowed_misses);
int btlbf_interleave_mates(const char* seq1, const uint64_t* starts1, const char* seq2, const uint64_t* starts2,
                           uint64_t n_pairs, char* out, uint64_t* out_starts, int mem, int device, void* stream);
int btlbf_mibf_classify_tally(const btlbf_mibf_hit* hits, const uint32_t* n_hits, const uint32_t* sat_count,
                              const uint32_t* eval_count, uint64_t n_rows, uint32_t max_results, uint64_t n_ids,
                              uint64_t* best, uint64_t* any, uint64_t* totals6, int mem, int device, void* stream);

/* ---- multi-GPU hash-range sharding ------------------------------------------------
 * The M-bit filter is cut into n_shards contiguous bit ranges; shard g (btlbf_create_shard) holds
 * positions [g*M/n, (g+1)*M/n).  Routing is by POSITION, so the concatenated shard bodies are the
 * single-filter body bit for bit.
 * positions_seqs: hash a device-resident sequence buffer with f's parameters and, instead of probing,
 *   append every probe of every clean window to the bucket of the shard that owns its position.
 *   buckets = n_shards regions of bucket_cap uint64_t in one device array; an entry is the position
 *   LOCAL to the owning shard.  tags (same shape, may be NULL) receives the probe id p*hash_num + i
 *   (p = window offset) so that routed answers can be matched up again.  bucket_counts[n_shards]
 *   (device) is zeroed by the call and receives the fill; a count above bucket_cap means entries
 *   were dropped and the caller must retry with a larger capacity.  valid_bits (device, may be
 *   NULL) is the usual per-window bitmap.
 * insert_positions / test_positions act on local positions of this shard (test: one byte 0/1 each).
 * and_answers: origin side of a sharded query -- answers[i] belongs to probe tags[i]; a 0 answer
 *   clears the bit of window tags[i]/hash_num in hit_bits (which starts as a copy of valid_bits).
 * positions_seqs, insert_positions, test_positions and every btlbf_route_* / btlbf_apply_* / btlbf_resolve_seqs /
 * btlbf_owner_scratch_bytes call below: EINVAL before any HIP call for a wide counting filter. */
int btlbf_positions_seqs(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                         unsigned n_shards, uint64_t* buckets, uint64_t* tags, uint64_t bucket_cap,
                         uint64_t* bucket_counts, uint64_t* valid_bits, void* stream);
int btlbf_insert_positions(btlbf_filter* f, const uint64_t* local_pos, uint64_t n, void* stream);
int btlbf_test_positions(btlbf_filter* f, const uint64_t* local_pos, uint64_t n, uint8_t* out,
                         void* stream);
int btlbf_and_answers(const uint64_t* tags, const uint8_t* answers, uint64_t n, unsigned hash_num,
                      uint64_t* hit_bits, int device, void* stream);
/* ---- multi-GPU on the partitioned pipeline (large batches) -----------------------
 * Needs a filter whose GLOBAL size and shard count are powers of two (at least 2^29 bits / 2^26 counters).
 * An entry is the 32-bit offset of a position inside its level-0 bin and an origin stages at most 1024 bins,
 * so one routing pass covers a WINDOW of at most 2^42 positions: a larger filter (BASELINE config 4: 2^43
 * bits on 8 GPUs) has several windows, each owned by n_shards / n_windows consecutive shards, and the same
 * reads are routed once per window (btlbf_route_windows; position semantics BloomFilter.hpp:190).  A window
 * is cut into B level-0 bins (512, or 1024 when a window has more than 2^41 positions); the s-th shard of
 * a window owns its bins [s*B/spw, (s+1)*B/spw).  All pointers are device pointers.
 *  route_windows: how many windows this geometry has, and how many shards own each.
 *  route_plan : byte sizes of ONE origin->owner block for a buffer of `plan_len` bytes.  Every rank
 *               must plan with the same plan_len (e.g. the maximum over ranks) so that blocks have one
 *               size and the exchange is a fixed-size all-to-all.
 *  route_seqs : origin.  Hash the buffer and partition every probe position inside `window` into the window's
 *               bins: send_ent / send_cnt receive shards_per_window consecutive blocks (block i goes to shard
 *               window*shards_per_window + i).
 *               query != 0 additionally writes valid_bits and initialises hit_bits = valid_bits;
 *               counts[0] (optional) += clean windows.  Entries that cannot be staged are appended to
 *               spill_list as global positions.  counts and spill_count ACCUMULATE over calls (zero
 *               them once per pass): no host round trip per batch is needed, so the exchange of one
 *               batch can overlap the hashing of the next.
 *  apply_routed: owner.  recv_ent / recv_cnt hold n_blocks blocks (one per origin, any order); they are
 *               split down to segments and ORed into (query == 0) or tested against (query != 0) this
 *               shard in LDS.  Positions found clear are appended to fail_list as GLOBAL positions
 *               (fail_count must be zeroed by the caller).
 *  route_geometry / apply_routed_bins: the same, group by group.  out4 = {level-0 bins per shard B/n,
 *               regions per bin, chunks (128 bytes) per region, bins per group}: a block is laid out
 *               [bin][region][chunk], so the bins of one group are a contiguous slice of every block
 *               (entries: bins*regions*chunks*128 bytes, counts: bins*regions*4 bytes).  An owner may
 *               receive and apply its bins a group at a time -- recv_ent / recv_cnt then hold, per
 *               origin block, only bins [first_bin, first_bin + n_bins) (whole groups) -- so that the
 *               receive buffers are a fraction of a block set and the exchange of one group overlaps
 *               the apply of the previous one.  n_blocks = 0 in route_geometry means n_shards.
 *  apply_spill : owner.  Insert / test explicit global positions (the gathered spill lists); positions
 *               of other shards are ignored.
 *  resolve_seqs: origin.  Clear the hit bit of every window that owns one of the (gathered) failed
 *               global positions. */
int btlbf_route_plan(btlbf_filter* f, uint64_t plan_len, const btlbf_layout* layout, unsigned n_shards,
                     uint64_t* ent_bytes_per_shard, uint64_t* cnt_bytes_per_shard);
int btlbf_route_windows(btlbf_filter* f, unsigned n_shards, unsigned* n_windows, unsigned* shards_per_window);
int btlbf_route_seqs(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                     uint64_t plan_len, unsigned n_shards, unsigned window, int query, void* send_ent,
                     void* send_cnt, uint64_t* hit_bits, uint64_t* valid_bits, uint64_t* counts,
                     uint64_t* spill_list, uint64_t spill_cap, uint64_t* spill_count, void* stream);
int btlbf_apply_routed(btlbf_filter* f, const void* recv_ent, const void* recv_cnt, unsigned n_blocks,
                       uint64_t plan_len, const btlbf_layout* layout, unsigned n_shards, int query,
                       uint64_t* fail_list, uint64_t fail_cap, uint64_t* fail_count, void* stream);
int btlbf_route_geometry(btlbf_filter* f, uint64_t plan_len, const btlbf_layout* layout, unsigned n_shards,
                         unsigned n_blocks, uint32_t* out4);
/* Bytes of partition scratch the OWNER side (btlbf_apply_routed / btlbf_apply_routed_bins) allocates inside the filter
 * for batches planned with `plan_len`, `n_blocks` origin blocks (0: n_shards): lets the caller size its batches from
 * the free HBM exactly instead of by rule of thumb (sharded.py plans BASELINE config 4 -- 1 TiB on 8 GPUs, SURVEY 8e --
 * with four batches per pass instead of five that way).  No device work. */
int btlbf_owner_scratch_bytes(btlbf_filter* f, uint64_t plan_len, const btlbf_layout* layout, unsigned n_shards,
                              unsigned n_blocks, uint64_t* bytes);
int btlbf_apply_routed_bins(btlbf_filter* f, const void* recv_ent, const void* recv_cnt, unsigned n_blocks,
                            unsigned first_bin, unsigned n_bins, uint64_t plan_len, const btlbf_layout* layout,
                            unsigned n_shards, int query, uint64_t* fail_list, uint64_t fail_cap,
                            uint64_t* fail_count, void* stream);
int btlbf_apply_spill(btlbf_filter* f, const uint64_t* global_pos, uint64_t n, int query, uint64_t* fail_list,
                      uint64_t fail_cap, uint64_t* fail_count, void* stream);
int btlbf_resolve_seqs(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                       const uint64_t* fail_list, uint64_t n_fail, uint64_t* hit_bits, void* stream);

/* Planning only, no device needed: the READ GRID pass A of the partitioned pipeline uses for fixed-length reads of
   read_len bases with `level0_bins` level-0 bins: out4 = { reads per tile, groups of 8
   window starts per read, bytes a read occupies in the LDS tile, bytes of LDS the tile image takes }; all zero
   when plain tiles are used instead (ragged input, reads too short / too long, no gain). */
int btlbf_plan_read_grid(unsigned kmer_size, unsigned hash_num, unsigned read_len, unsigned level0_bins,
                         uint32_t* out4);

/* Planning only, no device needed: pass A's front end for plain ntHash at kmer_size with `level0_bins` level-0 bins:
   out4 = { 1 if pass A fits the LDS (0: the partitioned modes hand the call to the direct kernels), bytes of dynamic
   LDS it asks for with a plain tile, 1 if the positional seed table is used, words of the ragged layout's start
   bitmap (0: no room, the plain schedule runs) }.  See "k-mer sizes" above. */
int btlbf_plan_pass_a(unsigned kmer_size, unsigned hash_num, unsigned level0_bins, uint32_t* out4);

/* Planning only, no device needed: what btlbf_set_spaced_seeds, btlbf_hash_seqs and btlbf_mibf_create would make of
   these spaced seeds.  out2 = { bytes of LDS per workgroup the direct kernels need with them (0 when refused for
   another reason), bytes available }.  Returns BTLBF_EINVAL, with the same message, exactly when those calls do. */
int btlbf_plan_spaced_lds(unsigned kmer_size, const char* const* seeds, unsigned n_seeds, unsigned h2, uint32_t* out2);

/* number of set bits in a device buffer of nbytes (multiple of 8, e.g. a hit bitmap); synchronises the stream */
int btlbf_popcount_bits(const void* dev_buf, uint64_t nbytes, uint64_t* out, int device, void* stream);

/* ---- support ------------------------------------------------------------------------------------
 * synthetic reads of SURVEY.md 8d written to device memory: n reads x read_len bytes */
int btlbf_synth_reads(char* dev_out, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                      unsigned read_len, int device, void* stream);
/* bare random-access ceilings on the filter's own array (SURVEY.md 8d "measured ceiling"):
 * kind 0 = independent 4-byte loads, 1 = 4-byte atomicOr (sets bits: clear the filter afterwards),
 * at uniformly random 64-byte-aligned offsets; about n_access accesses, the exact number is
 * returned in *n_done; *seconds = kernel time from HIP events.  Wide counting filters: EINVAL. */
int btlbf_microbench(btlbf_filter* f, int kind, uint64_t n_access, uint64_t* n_done, double* seconds);

/* per-sequence totals of the per-window bitmaps that btlbf_contains_seqs / btlbf_insert_and_check_seqs
 * produce: hits_out[s] = windows of sequence s whose bit is set in hit_bits, valid_out[s] (optional) =
 * its clean windows (valid_bits == NULL: all of its len-k+1 windows).  This is what read classifiers
 * built on the reference do per read with an ntHashIterator loop and a counter.  Device pointers
 * (mem == BTLBF_DEVICE) or host buffers; layout as for the call that made the bitmaps. */
int btlbf_count_per_seq(const uint64_t* hit_bits, const uint64_t* valid_bits, uint64_t len,
                        const btlbf_layout* layout, unsigned kmer_size, uint32_t* hits_out, uint32_t* valid_out,
                        int mem, int device, void* stream);

/* ---- FASTA / FASTQ ingestion -------------------------------------------------
 * Replaces the reference's toy loaders: Tests/AdHoc/ParallelFilter.cpp:104-122 (loadBf: header line +
 * one sequence line, an ntHashIterator per line) and swig/writeBloom_rolling.cpp:18-59
 * (contigsToBloom: the lines of a FASTA record are concatenated, then insertSeq).
 * Input may be gzip-compressed.  Format by the first byte: '>' FASTA, '@' FASTQ (4-line records),
 * anything else = one sequence per line. */
enum btlbf_fastx_flags {
	BTLBF_FASTX_RECORDS = 0,  /* the wrapped lines of a FASTA record form ONE sequence (contigsToBloom) */
	BTLBF_FASTX_LINES = 1,    /* every sequence line is its own sequence (loadBf) */
	BTLBF_FASTX_PAGEABLE = 2, /* do not pin the host buffers */
	BTLBF_FASTX_WHOLE = 4     /* never cut a sequence: one that does not fit the rest of a batch opens the next batch, and
	                             one longer than a whole batch is an error (EINVAL from btlbf_fastx_next, the message
	                             names the record).  batch_bytes may then be as small as the longest sequence.  An empty
	                             sequence line of a FASTQ record is delivered as an empty sequence (without the flag it
	                             is skipped), so that sequences and records correspond one to one */
};
typedef struct btlbf_fastx btlbf_fastx;

/* streaming parser: batches of at most batch_bytes sequence bytes (0 = 256 MiB) in the ragged layout
 * of btlbf_layout; a sequence longer than a batch is cut with a k-1 base overlap so that every
 * window appears in exactly one batch */
int btlbf_fastx_open(btlbf_fastx** r, const char* path, uint32_t flags, uint32_t k, uint64_t batch_bytes);
/* *bases (n_bases bytes) and *starts (n_seqs+1 offsets) stay valid until the call after the next
 * one; n_seqs == 0 at end of input.  A read error -- an I/O error, a truncated or corrupt gzip stream -- is
 * BTLBF_EIO from the call that meets it (the message names the file and the cause): that call delivers no
 * sequences, the batches delivered before it stay delivered, and btlbf_fastx_records keeps its count */
int btlbf_fastx_next(btlbf_fastx* r, const char** bases, uint64_t* n_bases, const uint64_t** starts,
                     uint64_t* n_seqs);
/* one of several readers over the same UNCOMPRESSED file (parallel parsing): delivers the records that
 * START in byte range [begin, end); the ranges of all readers must tile the file.  fmt: 1 = FASTA,
 * 2 = FASTQ (4-line), 3 = one sequence per line.  btlbf_insert_fastx / btlbf_contains_fastx do this
 * internally (BTLBF_FASTX_THREADS, default min(8, cores)). */
int btlbf_fastx_open_range(btlbf_fastx** r, const char* path, uint32_t flags, uint32_t k, uint64_t batch_bytes,
                           int fmt, uint64_t begin, uint64_t end);
uint64_t btlbf_fastx_records(const btlbf_fastx* r); /* records seen so far */
void btlbf_fastx_close(btlbf_fastx* r);

typedef struct btlbf_fastx_stats {
	uint64_t n_records;  /* FASTA / FASTQ records (lines, for plain input) */
	uint64_t n_bases;    /* sequence bytes sent to the GPU (overlaps of cut sequences included) */
	uint64_t n_windows;  /* contains: clean k-mer windows tested */
	uint64_t n_hits;     /* contains: windows found in the filter */
	uint64_t n_batches;
	double seconds_parse; /* host time inside the parser */
	double seconds_total; /* wall time of the call */
} btlbf_fastx_stats;

/* whole file -> filter: pinned double buffers, copies on a copy stream, kernels on a compute stream;
 * the host parses batch i+1 while batch i is copied and hashed.  stats may be NULL. */
int btlbf_insert_fastx(btlbf_filter* f, const char* path, uint32_t flags, uint64_t batch_bytes,
                       btlbf_fastx_stats* stats);
int btlbf_contains_fastx(btlbf_filter* f, const char* path, uint32_t flags, uint64_t batch_bytes,
                         btlbf_fastx_stats* stats);

/* ---- read classification from FASTA / FASTQ files ---------------------------------------------------------
 * What a caller of the reference writes around MIBFQuerySupport<T>::query (MIBFQuerySupport.hpp:95-130): read the
 * file(s), classify every read or pair, keep per-read results and reads per id.  Three modes:
 *   path2 == NULL, no flag            : single reads (mibf_classify_seqs); a row is a record;
 *   path2 != NULL                     : record i of path1 and record i of path2 are pair i (mibf_classify_pairs);
 *   path2 == NULL, CLASSIFY_INTERLEAVED: records 2i and 2i + 1 of path1 are pair i.
 * path2 together with the flag is EINVAL.  flags may also hold BTLBF_FASTX_LINES / BTLBF_FASTX_PAGEABLE;
 * BTLBF_FASTX_WHOLE is always set: a row is a whole read, so batch_bytes (0 = 64 MiB) must hold the longest record.
 * Rows come out in file order, and equal mibf_classify_seqs / _pairs on the same reads row for row.
 * open : checks, before any HIP call and before the miBF is looked at: null arguments (path2 may be null), max_results == 0,
 *   n_ids == 0, both pairing modes, an unreadable file (EIO); then n_ids against the id type as mibf_classify_seqs.  The
 *   tables are uploaded once.  Each file gets one sequential parser (btlbf_fastx_open / _next) on a thread of its own --
 *   at most two threads, no byte-range readers -- that fills pinned batches ahead of the caller, a bounded number in
 *   flight; the two files' batches are cut by bytes and zipped on the host record by record (csrc/mibf_zip.hpp).
 * next : one batch: the bases and offsets go to the device on a copy stream; on the compute stream, for two files,
 *   interleave_mates, then mibf_classify_seqs / _pairs (BTLBF_DEVICE), mibf_classify_tally into the handle's running
 *   device totals, and the copy of the four result arrays into one of two pinned result sets.  mibf_classify_* plans
 *   on the host and synchronises its stream, so the call returns with its batch finished; the parser threads parse the
 *   next two batches meanwhile.  *first_row is contiguous from 0 over successive calls; *n_rows == 0 at end of input.
 *   The result pointers stay valid until the call after the next one (btlbf_fastx_next's rule).  hits may be passed as
 *   NULL together with the other three result pointers: no per-row result then leaves the device (the whole-file call
 *   does this).  A FASTQ record with an empty sequence line is a row (an empty read, or an empty mate); a FASTA record
 *   without sequence lines is not.  Whatever classify reports (an id index >= n_ids,
 *   ENOMEM for a row beyond the scratch budget) and whatever the parser reports (a record longer than a batch) comes
 *   back unchanged.  Unequal record counts of the two files, or an odd count in interleaved mode, are EFORMAT from the
 *   call that reaches the end of input; rows delivered before stay delivered.
 * tally : the running totals so far, in the layout of mibf_classify_tally (best / any: n_ids entries).
 * classify_fastx : open, next until the end without per-row copies, tally, close.  stats (optional): n_records,
 *   n_bases, n_batches, seconds_parse (the slower parser), seconds_total; n_windows / n_hits stay 0. */
enum { BTLBF_CLASSIFY_INTERLEAVED = 1u << 8 };
typedef struct btlbf_mibf_fastx btlbf_mibf_fastx;
int btlbf_mibf_classify_fastx_open(btlbf_mibf_fastx** c, btlbf_mibf* m, const char* path1, const char* path2,
                                   uint32_t flags, const btlbf_mibf_classify_params* p, const double* per_frame_prob,
                                   const uint32_t* min_count_per_id, uint64_t n_ids, uint64_t batch_bytes);
int btlbf_mibf_classify_fastx_next(btlbf_mibf_fastx* c, uint64_t* first_row, uint64_t* n_rows,
                                   const btlbf_mibf_hit** hits, const uint32_t** n_hits, const uint32_t** sat_count,
                                   const uint32_t** eval_count);
int btlbf_mibf_classify_fastx_tally(btlbf_mibf_fastx* c, uint64_t* best, uint64_t* any, uint64_t* totals6);
void btlbf_mibf_classify_fastx_close(btlbf_mibf_fastx* c);
int btlbf_mibf_classify_fastx(btlbf_mibf* m, const char* path1, const char* path2, uint32_t flags,
                              const btlbf_mibf_classify_params* p, const double* per_frame_prob,
                              const uint32_t* min_count_per_id, uint64_t n_ids, uint64_t batch_bytes, uint64_t* best,
                              uint64_t* any, uint64_t* totals6, btlbf_fastx_stats* stats);

/* ---- miBF construction from FASTA / FASTQ files (stages 1-4) ------------------------------------------------
 * What a caller of the reference's MIBFConstructSupport writes around insertBVColli / getEmptyMIBF / insertMIBF /
 * insertSaturation: read the reference sequences, size the bit vector (calcOptimalSize, MIBloomFilter.hpp:84-88), give
 * every sequence its id, run the passes in order.  mibf_build_fastx does that over files, in argument order, records in
 * file order:
 *   pass 0 (count)  : only when bits == 0 && expected_entries == 0: the clean windows of all files
 *                     (count_windows_seqs per batch) are the entries the bit vector is sized for;
 *   pass 1 (stage 1): a bit filter of `bits` bits (plain ntHash with hash_num values, or the spaced seeds with h2 = 1),
 *                     every sequence inserted (insert_seqs per batch); it also counts the records and finds the longest;
 *   stage 2         : mibf_create;
 *   pass 2          : mibf_insert_ids_seqs per batch, with the ids made on the device;
 *   pass 3          : mibf_saturate_seqs per batch, unless BTLBF_MIBF_SAT_NONE.
 * Every pass reads the files again.  One sequential parser per file runs ahead on a thread of its own (the
 * classifier's arrangement); a parser batch goes to one of two device slots on a copy stream, so that batch j + 1 is
 * copied while the stage call of batch j, which plans on the host and synchronises the compute stream, runs.
 * A sequence is what btlbf_fastx_open(path, flags | BTLBF_FASTX_WHOLE, k, batch_bytes) delivers (flags: BTLBF_FASTX_LINES,
 * BTLBF_FASTX_PAGEABLE): whole records only -- batch_bytes (0 = 64 MiB) must hold the longest record, and a longer one is
 * the parser's EINVAL, naming the record.  Wrapped FASTA lines are one sequence unless BTLBF_FASTX_LINES is set; a FASTQ
 * record with an empty sequence line is a sequence (and, per record, takes an id); a FASTA record without sequence lines
 * is not.  Record names are not delivered: there is no id-to-name table.  A batch never spans two files.
 * ids: BTLBF_MIBF_ID_PER_FILE: every sequence of file j gets first_id + j; BTLBF_MIBF_ID_PER_RECORD: sequence r, counted
 * over all files in order, gets first_id + r.
 * The result, with S = all sequences in that order, with their ids:
 *   E1  the stage-1 body is byte for byte that of btlbf_insert_seqs of S into an empty filter of that size, seeds and k;
 *   E2  after pass 2, data and counts equal ONE btlbf_mibf_insert_ids_seqs call over S (its ascending-value rule makes
 *       the result independent of batch cuts; a cut record would change the counts, hence whole records);
 *   E3  SAT_SERIAL equals ONE BTLBF_ORDER_SERIAL call over S;
 *   E4  SAT_PARALLEL equals one BTLBF_ORDER_PARALLEL call per parser batch, in order: the batches are those
 *       btlbf_fastx_open(path, flags | BTLBF_FASTX_WHOLE, k, batch_bytes) / _next deliver for each file in turn, so the
 *       result depends on batch_bytes; report->sat_counts4 sums the counts4 of those calls;
 *   E5  bits == 0 gives btlbf_mibf_optimal_size(entries, hash_num, occupancy), entries being expected_entries or pass 0's
 *       count: the reference's arithmetic, the same double operations in the same order.
 * Checked at entry, before any HIP call and with nothing allocated: null or empty arguments; an unreadable path, any of
 * them (EIO, naming it); id_bytes other than 2 / 4; first_id == 0; per file, first_id + n_paths - 1 at or above the
 * saturation mask 1 << (8 * id_bytes - 1); an unknown id_mode or saturation; occupancy outside (0, 1) when bits == 0; a
 * `bits` that is 0 after sizing or no multiple of 8; hash_num outside 1..8; kmer_size == 0; seeds whose count or length
 * disagree with hash_num / kmer_size; for SAT_PARALLEL a batch_bytes whose worst case -- every window of a batch a
 * mutation, every probe a saturation -- does not fit the shares the parallel call gives the two lists of scratch_bytes
 * (0 = the default 2 GiB): ENOMEM, the message states the budget that would do (mibf_parallel_budget, csrc/mibf_plan.hpp).
 * Checked at the end of pass 1, before stage 2: per record, the last id at or above the mask (EINVAL); the longest
 * record beyond what one insert batch, or with SAT_SERIAL one serial saturation batch, holds under the budget (ENOMEM,
 * stating the budget needed).  Read errors are EIO.  On any failure *out and *stage1_out are NULL and nothing is left
 * allocated.  stage1_out may be NULL (the filter is then destroyed; store it with btlbf_store to load the miBF again);
 * report and records_per_file[n_paths] are optional.
 * mibf_optimal_size  : calcOptimalSize (MIBloomFilter.hpp:84-88), pure host arithmetic.
 * count_windows_seqs : out2 = {windows, clean windows} of the sequences of a buffer (layout as btlbf_insert_seqs; NULL:
 *                     one sequence).  A window is k bytes inside one sequence; it is clean when each of them is a base
 *                     the hash kernels accept -- don't-care positions of spaced seeds included, so the count depends on
 *                     k alone.  No hashing.  out2 lives in memory space mem; a DEVICE call returns with the work queued.
 * count_windows_fastx: the same over a file; stats->n_windows = clean windows, n_hits = windows. */
enum { BTLBF_MIBF_ID_PER_FILE = 0, BTLBF_MIBF_ID_PER_RECORD = 1 };
enum { BTLBF_MIBF_SAT_NONE = 0, BTLBF_MIBF_SAT_SERIAL = 1, BTLBF_MIBF_SAT_PARALLEL = 2 };
typedef struct btlbf_mibf_build_params {
	unsigned kmer_size, hash_num; /* with seeds: hash_num == n_seeds */
	const char* const* seeds;
	unsigned n_seeds;
	unsigned id_bytes; /* 2 | 4 */
	uint64_t bits;             /* 0: btlbf_mibf_optimal_size(entries, hash_num, occupancy) */
	uint64_t expected_entries; /* 0: counted (pass 0) */
	double occupancy;
	int id_mode;
	uint32_t first_id;
	int saturation;
	uint32_t fastx_flags;
	uint64_t batch_bytes, scratch_bytes;
	int device;
} btlbf_mibf_build_params;
typedef struct btlbf_mibf_build_report {
	uint64_t entries; /* what the bit vector was sized for; 0 when bits was given */
	uint64_t bits, pop;
	uint64_t n_records, n_ids; /* sequences over all files; ids assigned (n_paths or n_records) */
	uint64_t longest_record, n_bases;
	uint64_t windows, clean_windows; /* pass 0; 0 when it did not run */
	uint64_t sat_counts4[4];         /* {clean windows, found, mutated, saturated} summed over pass 3's calls */
	uint64_t batches[4];             /* per pass */
	double seconds[4], seconds_parse[4];
	double seconds_total;
} btlbf_mibf_build_report;
int btlbf_mibf_build_fastx(btlbf_mibf** out, btlbf_filter** stage1_out, const char* const* paths, unsigned n_paths,
                           const btlbf_mibf_build_params* p, btlbf_mibf_build_report* report, uint64_t* records_per_file);
uint64_t btlbf_mibf_optimal_size(uint64_t entries, unsigned hash_num, double occupancy);
int btlbf_count_windows_seqs(unsigned kmer_size, const char* seq, uint64_t len, const btlbf_layout* layout, uint64_t* out2,
                             int mem, int device, void* stream);
int btlbf_count_windows_fastx(const char* path, unsigned kmer_size, uint32_t flags, uint64_t batch_bytes, int device,
                              btlbf_fastx_stats* stats);

/* ---- read screen: every read against several bit filters in one pass ------------------------------------------
 * What a caller writes around BloomFilter::contains to screen reads against a set of filters (a genome, contaminant
 * sets): per read and filter, how many of the read's k-mers the filter holds.  One fused kernel hashes every window
 * once and probes all filters with it (csrc/screen_kernels.hip); more than 8 filters run in groups, hashing once per
 * group.
 * screen_seqs : per sequence s of the buffer (layout as btlbf_contains_seqs; NULL: the buffer is one sequence; read_len:
 *   len / read_len rows) valid[s] = its clean windows and hits[s * n_filters + j] = those of them all of whose bits
 *   are set in filters[j].  DEFINITION: hits[:, j] and valid equal what btlbf_contains_seqs on filters[j] followed by
 *   btlbf_count_per_seq returns for the same buffer and layout.  pass_bits (may be NULL): bit j of pass_bits[s] is set
 *   iff valid[s] > 0 && hits >= p->min_hits && (double)hits >= p->min_fraction * (double)valid (one IEEE double
 *   multiply, one compare).  The filters are read and never changed; the call always runs the fused direct kernel, never
 *   the partitioned pipeline, whatever the filters' query mode.
 *   Refused with BTLBF_EINVAL before any HIP call, outputs untouched: a null argument (pass_bits excepted; seq may be
 *   null when len == 0); n_filters == 0 or > BTLBF_SCREEN_MAX_FILTERS; a null handle, or the same handle twice; a
 *   min_fraction outside [0, 1] or NaN; a mem that is neither space; a len that is no multiple of read_len; and then,
 *   looking at the filters: one that is not BTLBF_BLOOM (counting filters are not screened), or is a shard; filters on
 *   different devices; filters that differ in kmer_size, in hash_num, or in their spaced seeds (seed strings and h2).
 *   Every filter's internal lock is held for the whole call, taken in ascending handle address, so that two threads
 *   screening overlapping sets cannot deadlock.  A pending btlbf_clear is carried out first: a fresh or just-cleared
 *   filter's column is all zeros.  mem / stream as in btlbf_contains_seqs: BTLBF_HOST stages and returns with the
 *   results in place; BTLBF_DEVICE runs on the caller's stream and returns with the work queued (the per-window bitmaps
 *   it reduces live in scratch one of the filters owns, handed from call to call in stream order by an event).  Every
 *   element of hits, valid and a non-NULL pass_bits is written, and nothing beyond them.
 * screen_tally : the summary of rows, ADDED to the caller's counts (as btlbf_mibf_classify_tally): passed[j] += rows
 *   whose bit j is set; best[j] += rows whose passing filter with the most hits is j, ties going to the lowest j;
 *   totals4 += {rows, rows passing none, rows passing two or more, rows with valid == 0}.  A DEVICE call returns with
 *   the work queued.
 * screen_fastx_* : the same over one FASTA / FASTQ file (gzip or not): rows = records, in file order.  Read pairs (two
 *   files, an interleaved file) are not handled here.
 *   open : the checks of screen_seqs in the same order -- those that do not look at the filters first, then an unreadable
 *     path (EIO), then the filters; a device that is not there is BTLBF_EHIP.  The file gets one sequential parser on a thread of its own (the file classifier's
 *     reader, csrc/fastx_side.hpp) with BTLBF_FASTX_WHOLE always set (flags: BTLBF_FASTX_LINES, BTLBF_FASTX_PAGEABLE), so
 *     batch_bytes (0 = 64 MiB) must hold the longest record.
 *   next : one parser batch: bases and offsets go to one of two device slots on a copy stream; on the compute stream
 *     screen_seqs (BTLBF_DEVICE) under the filters' locks, screen_tally into the handle's running device totals, and the
 *     copy of the three result arrays into one of two pinned result sets; the call returns with its batch finished, the
 *     parser thread parses ahead meanwhile.  *first_row is contiguous from 0; *n_rows == 0 at end of input.  The result
 *     pointers stay valid until the call after the next one.  hits == NULL together with the other two result pointers:
 *     no per-row copy.  Every row equals screen_seqs over the same reads from memory.  Parser errors come back unchanged
 *     (BTLBF_EIO for a truncated gzip stream, EINVAL naming the record for one longer than batch_bytes) from the call
 *     that meets them; rows delivered before stay delivered.  Any error of a batch (the parser's, ENOMEM, a HIP error)
 *     ends the input: every later call returns it again, so that first_row never skips a batch.
 *   tally : the running totals so far, in screen_tally's layout.
 *   screen_fastx : open, next until the end without per-row copies, tally, close.  stats (optional): n_records, n_bases,
 *     n_batches, n_windows (the sum of valid), seconds_parse, seconds_total; n_hits stays 0. */
enum { BTLBF_SCREEN_MAX_FILTERS = 16 };
typedef struct btlbf_screen_params {
	double min_fraction;
	uint32_t min_hits;
	uint32_t reserved;
} btlbf_screen_params;
int btlbf_screen_seqs(btlbf_filter* const* filters, unsigned n_filters, const char* seq, uint64_t len,
                      const btlbf_layout* layout, const btlbf_screen_params* p, uint32_t* hits, uint32_t* valid,
                      uint32_t* pass_bits, int mem, void* stream);
int btlbf_screen_tally(const uint32_t* hits, const uint32_t* valid, const uint32_t* pass_bits, uint64_t n_rows,
                       unsigned n_filters, uint64_t* passed, uint64_t* best, uint64_t* totals4, int mem, int device,
                       void* stream);
typedef struct btlbf_screen_file btlbf_screen_file;
int btlbf_screen_fastx_open(btlbf_screen_file** c, btlbf_filter* const* filters, unsigned n_filters, const char* path,
                            uint32_t flags, const btlbf_screen_params* p, uint64_t batch_bytes);
int btlbf_screen_fastx_next(btlbf_screen_file* c, uint64_t* first_row, uint64_t* n_rows, const uint32_t** hits,
                            const uint32_t** valid, const uint32_t** pass_bits);
int btlbf_screen_fastx_tally(btlbf_screen_file* c, uint64_t* passed, uint64_t* best, uint64_t* totals4);
void btlbf_screen_fastx_close(btlbf_screen_file* c);
int btlbf_screen_fastx(btlbf_filter* const* filters, unsigned n_filters, const char* path, uint32_t flags,
                       const btlbf_screen_params* p, uint64_t batch_bytes, uint64_t* passed, uint64_t* best,
                       uint64_t* totals4, btlbf_fastx_stats* stats);

/* ---- k-mer cardinality and spectrum: how large must the filter be? ---------------------------------------------
 * Every constructor above takes a size; this estimates the number it is computed from -- F0, the distinct k-mers of the
 * input, and f1, f2, ..., the distinct k-mers that occur once, twice, ... -- from a sampled, bucketed sketch built in
 * HBM by one fused kernel (csrc/card_kernels.hip) and solved on the host.
 * THE SKETCH (tests hold the code to it bit for bit).  For every clean window w of the input (clean as everywhere in
 * this header): h0(w) = the canonical ntHash value (btlbf_hash_seqs with hash_num 1, no seeds); z = mix64(h0), mix64 the
 * splitmix64 finaliser written out at btlbf_digest (h0 = min(forward, reverse) is not uniform in its high bits);
 * w is SAMPLED iff sample_bits == 0 || (z >> (64 - sample_bits)) == 0; a sampled window adds 1 to
 * table[z & (2^table_bits - 1)].  The counters are uint32_t and saturate at 2^32 - 1: they never wrap.
 * totals3 = {windows, clean windows, sampled windows} (a window: k bytes inside one sequence, as
 * btlbf_count_windows_seqs counts them), accumulated on the device.
 *   sample_bits 0..32, table_bits 6..28 (the table takes 4 << table_bits bytes of HBM, plus a bit per counter),
 *   kmer_size 1..32768 (what btlbf_hash_seqs takes without seeds).  Spaced seeds are not offered.
 * create / destroy / clear : a sketch on `device`, all zero.  clear zeroes the table and the totals.
 * add_seqs : the windows of a buffer (layout, mem and stream as btlbf_insert_seqs) are added: BTLBF_HOST stages the
 *   buffer and returns with the work finished; BTLBF_DEVICE runs on the caller's stream and returns with the work
 *   queued.  Calls accumulate: two calls over two halves of a set of reads leave what one call over all leaves.
 * add_fastx : the same over a FASTA / FASTQ file, plain or gzip, in the file classifier's arrangement: one sequential
 *   parser (btlbf_fastx_open / _next) on a thread of its own, parser batches of batch_bytes (0 = 64 MiB, or what the
 *   test switch BTLBF_FASTX_DEV_BYTES says) that rotate through two device slots, the copy of batch j + 1 overlapping
 *   the kernel of batch j.  flags: BTLBF_FASTX_LINES, BTLBF_FASTX_PAGEABLE, BTLBF_FASTX_WHOLE.  Without
 *   BTLBF_FASTX_WHOLE a record that does not fit the rest of a batch is cut with the parser's k - 1 base overlap, so
 *   that every window is counted exactly once: the sketch does not depend on batch_bytes.  stats (optional):
 *   n_records, n_bases, n_batches, n_windows = clean windows and n_hits = sampled windows of this call, the seconds.
 *   Returns with the work finished.  A parser error (BTLBF_EIO for a truncated gzip stream) comes back unchanged; the
 *   batches before it stay added.
 * merge : dst[i] = min(dst[i] + src[i], 2^32 - 1) and the totals added; both of the same kmer_size, sample_bits,
 *   table_bits and device, else BTLBF_EINVAL.  The sketch of two inputs merged is the sketch of their concatenation.
 * download / upload : the 2^table_bits counters and totals3, to and from host memory (a sketch can be kept, or moved
 *   between GPUs and merged there).
 * histogram : t[i] = the number of counters equal to i for i < n_hist - 1, t[n_hist - 1] = those >= n_hist - 1;
 *   n_hist 3..8192; t is host memory.  One streaming pass over the table.
 * clear, merge, download, upload, histogram and estimate_now take no stream: they wait for ALL streams of the device
 * before they look at the table, and return with their work finished.
 * solve : pure host arithmetic, no HIP call, no GPU.  In double, in this order:  R = 2^table_bits;
 *   L = table_bits * log(2.0) - log((double)t[0]);  F0 = ldexp(L, table_bits + sample_bits);
 *   phi[i] = t[i] / (t[0] * L) - (sum_{j=1}^{i-1} j * t[i-j] * phi[j]) / (i * t[0])  for i = 1 .. n_hist - 2;
 *   f[i] = fabs(phi[i]) * F0;  f[0] = 0.  f holds n_hist - 1 doubles.  est->distinct = F0, singletons = f[1],
 *   occupancy = 1 - t[0] / R, overflow_buckets = t[n_hist - 1]; windows, clean_windows and sampled are 0 (estimate_now
 *   fills them from totals3).  t[0] == 0 (the table is full) is BTLBF_EINVAL -- raise table_bits or sample_bits -- and
 *   so is a histogram that does not sum to R; nothing is written then.  t[0] == R: F0 = 0 and every f is 0.
 *   Trust the estimate while the occupancy is roughly between 0.05 and 0.8; no limit is
 *   enforced.
 * estimate_now : histogram + solve.
 * Refused before any HIP call, with nothing allocated and no output written: a null argument (layout, stream and stats
 * may be null; seq when len == 0); kmer_size 0 or above 32768; sample_bits > 32; table_bits outside 6..28; n_hist outside
 * 3..8192; a mem that is neither space; a len that is no multiple of read_len (all BTLBF_EINVAL); an unreadable path
 * (BTLBF_EIO).  A call that returns BTLBF_OK has written every element of every output. */
typedef struct btlbf_card btlbf_card;
typedef struct btlbf_card_estimate {
	double distinct;   /* F0 */
	double singletons; /* f1 */
	double occupancy;  /* 1 - t[0] / 2^table_bits */
	uint64_t windows, clean_windows, sampled; /* totals3 (0 from btlbf_card_solve) */
	uint64_t overflow_buckets;                /* t[n_hist - 1] */
} btlbf_card_estimate;
int btlbf_card_create(btlbf_card** out, unsigned kmer_size, unsigned sample_bits, unsigned table_bits, int device);
void btlbf_card_destroy(btlbf_card* c);
int btlbf_card_clear(btlbf_card* c);
int btlbf_card_add_seqs(btlbf_card* c, const char* seq, uint64_t len, const btlbf_layout* layout, int mem, void* stream);
int btlbf_card_add_fastx(btlbf_card* c, const char* path, uint32_t flags, uint64_t batch_bytes, btlbf_fastx_stats* stats);
int btlbf_card_merge(btlbf_card* dst, const btlbf_card* src);
int btlbf_card_download(btlbf_card* c, uint32_t* table, uint64_t* totals3);
int btlbf_card_upload(btlbf_card* c, const uint32_t* table, const uint64_t* totals3);
int btlbf_card_histogram(btlbf_card* c, uint64_t* t, unsigned n_hist);
int btlbf_card_solve(const uint64_t* t, unsigned n_hist, unsigned sample_bits, unsigned table_bits,
                     btlbf_card_estimate* est, double* f);
int btlbf_card_estimate_now(btlbf_card* c, unsigned n_hist, btlbf_card_estimate* est, double* f);

#ifdef __cplusplus
}
#endif
#endif /* BTLBF_H */
