"""ctypes binding of the C ABI in include/btlbf.h (libbtlbf.so, hand-written HIP for gfx950).

There is no Python or CPU fallback: if the shared library is missing this module raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# BTLBF_LIB selects another build of the SAME library (diagnostic / sanitizer builds made by build.py with
# BTLBF_BUILD_TAG, tools/sanitize_host.sh); there is no other implementation to select
LIB_PATH = os.environ.get("BTLBF_LIB") or os.path.join(HERE, "libbtlbf.so")

HOST, DEVICE = 0, 1
BLOOM, COUNTING8, COUNTING16, COUNTING32, COUNTING64 = 0, 1, 2, 3, 4
# counting kind of a counter width in bits, and back (btlbf_counter_bytes)
COUNTING_KIND = {8: COUNTING8, 16: COUNTING16, 32: COUNTING32, 64: COUNTING64}
INCREMENT_MIN, INCREMENT_ALL = 0, 1
ORDER_PARALLEL, ORDER_SERIAL = 0, 1
OK, EINVAL, ENOMEM, EIO, EFORMAT, EHIP = range(6)
INSERT_AUTO, INSERT_DIRECT, INSERT_PARTITIONED = 0, 1, 2
FASTX_LINES, FASTX_PAGEABLE, FASTX_WHOLE, CLASSIFY_INTERLEAVED = 1, 2, 4, 1 << 8
MIBF_ID_PER_FILE, MIBF_ID_PER_RECORD = 0, 1
MIBF_SAT_NONE, MIBF_SAT_SERIAL, MIBF_SAT_PARALLEL = 0, 1, 2
SCREEN_MAX_FILTERS = 16
COMBINE_OR, COMBINE_AND, COMBINE_ANDNOT, COMBINE_ADD, COMBINE_MAX, COMBINE_MIN = range(6)
COMBINE_MAX_SRCS = 16
PROF_SLOTS = 10
CARD_SAMPLE_BITS, CARD_TABLE_BITS = 11, 22  # the defaults of the layers above the C ABI
PROF_NAMES = ["insert_direct", "query_direct", "insert_hash", "insert_split", "insert_apply", "query_hash",
              "query_split", "query_test", "query_resolve", "other"]


class Layout(C.Structure):
    _fields_ = [("starts", C.c_void_p), ("n_seqs", C.c_uint64), ("read_len", C.c_uint32)]


class FastxStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_bases", C.c_uint64), ("n_windows", C.c_uint64),
                ("n_hits", C.c_uint64), ("n_batches", C.c_uint64), ("seconds_parse", C.c_double),
                ("seconds_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MibfClassifyParams(C.Structure):
    _fields_ = [("extra_count", C.c_double), ("extra_frame_limit", C.c_uint32), ("max_miss", C.c_uint32),
                ("min_count", C.c_uint32), ("best_hit_agree", C.c_uint32), ("max_results", C.c_uint32)]


class ScreenParams(C.Structure):
    _fields_ = [("min_fraction", C.c_double), ("min_hits", C.c_uint32), ("reserved", C.c_uint32)]


class CardEstimate(C.Structure):
    _fields_ = [("distinct", C.c_double), ("singletons", C.c_double), ("occupancy", C.c_double), ("windows", C.c_uint64),
                ("clean_windows", C.c_uint64), ("sampled", C.c_uint64), ("overflow_buckets", C.c_uint64)]


class MibfBuildParams(C.Structure):
    _fields_ = [("kmer_size", C.c_uint), ("hash_num", C.c_uint), ("seeds", C.POINTER(C.c_char_p)), ("n_seeds", C.c_uint),
                ("id_bytes", C.c_uint), ("bits", C.c_uint64), ("expected_entries", C.c_uint64), ("occupancy", C.c_double),
                ("id_mode", C.c_int), ("first_id", C.c_uint32), ("saturation", C.c_int), ("fastx_flags", C.c_uint32),
                ("batch_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64), ("device", C.c_int)]


class MibfBuildReport(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("bits", C.c_uint64), ("pop", C.c_uint64), ("n_records", C.c_uint64),
                ("n_ids", C.c_uint64), ("longest_record", C.c_uint64), ("n_bases", C.c_uint64), ("windows", C.c_uint64),
                ("clean_windows", C.c_uint64), ("sat_counts4", C.c_uint64 * 4), ("batches", C.c_uint64 * 4),
                ("seconds", C.c_double * 4), ("seconds_parse", C.c_double * 4), ("seconds_total", C.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if hasattr(getattr(self, k), "__len__") else getattr(self, k))
                for k, _ in self._fields_}


class BtlbfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("btlbf error %d: %s" % (code, msg))
        self.code = code


_lib = None

# name -> (restype, argtypes)
_P = C.c_void_p
_PROTOS = {
    "btlbf_last_error": (C.c_char_p, []),
    "btlbf_device_count": (C.c_int, []),
    "btlbf_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint64, C.c_uint, C.c_uint, C.c_uint, C.c_int]),
    "btlbf_create_shard": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint64, C.c_uint, C.c_uint, C.c_uint,
                                     C.c_uint, C.c_uint, C.c_int]),
    "btlbf_destroy": (C.c_int, [_P]),
    "btlbf_load": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.c_uint, C.c_int]),
    "btlbf_create_from_header": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.c_size_t, C.c_uint, C.c_int]),
    "btlbf_get_dfpr": (C.c_double, [_P]),
    "btlbf_set_dfpr": (None, [_P, C.c_double]),
    "btlbf_store": (C.c_int, [_P, C.c_char_p]),
    "btlbf_header": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "btlbf_store_shard": (C.c_int, [_P, C.c_char_p]),
    "btlbf_kind": (C.c_int, [_P]),
    "btlbf_counter_bytes": (C.c_uint, [_P]),
    "btlbf_size": (C.c_uint64, [_P]),
    "btlbf_size_bytes": (C.c_uint64, [_P]),
    "btlbf_local_bytes": (C.c_uint64, [_P]),
    "btlbf_hash_num": (C.c_uint, [_P]),
    "btlbf_kmer_size": (C.c_uint, [_P]),
    "btlbf_threshold": (C.c_uint, [_P]),
    "btlbf_get_n_entry": (C.c_uint64, [_P]),
    "btlbf_get_t_entry": (C.c_uint64, [_P]),
    "btlbf_set_n_entry": (None, [_P, C.c_uint64]),
    "btlbf_set_t_entry": (None, [_P, C.c_uint64]),
    "btlbf_device_ptr": (_P, [_P]),
    "btlbf_device": (C.c_int, [_P]),
    "btlbf_clear": (C.c_int, [_P, _P]),
    "btlbf_upload": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64]),
    "btlbf_download": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64]),
    "btlbf_set_insert_mode": (C.c_int, [_P, C.c_int, C.c_uint64]),
    "btlbf_release_scratch": (C.c_int, [_P]),
    "btlbf_set_profiling": (C.c_int, [_P, C.c_int]),
    "btlbf_get_profile": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint), C.c_int]),
    "btlbf_set_query_mode": (C.c_int, [_P, C.c_int]),
    "btlbf_set_spaced_seeds": (C.c_int, [_P, C.POINTER(C.c_char_p), C.c_uint, C.c_uint]),
    "btlbf_digest": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "btlbf_compare": (C.c_int, [_P, _P, C.POINTER(C.c_uint64)]),
    "btlbf_clone": (C.c_int, [C.POINTER(_P), _P]),
    "btlbf_combine": (C.c_int, [_P, C.POINTER(_P), C.c_uint, C.c_int, C.POINTER(C.c_uint64)]),
    "btlbf_fold": (C.c_int, [C.POINTER(_P), _P, C.c_uint64]),
    "btlbf_threshold_bits": (C.c_int, [C.POINTER(_P), _P, C.c_uint]),
    "btlbf_rank_create": (C.c_int, [C.POINTER(_P), _P]),
    "btlbf_rank_destroy": (None, [_P]),
    "btlbf_rank_ones": (C.c_uint64, [_P]),
    "btlbf_rank_words": (C.c_uint64, [_P]),
    "btlbf_rank_download": (C.c_int, [_P, _P]),
    "btlbf_rank_query": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P, _P, C.c_int, _P]),
    "btlbf_mibf_create": (C.c_int, [C.POINTER(_P), _P, C.c_uint]),
    "btlbf_mibf_destroy": (None, [_P]),
    "btlbf_mibf_size": (C.c_uint64, [_P]),
    "btlbf_mibf_bits": (C.c_uint64, [_P]),
    "btlbf_mibf_hash_num": (C.c_uint, [_P]),
    "btlbf_mibf_kmer_size": (C.c_uint, [_P]),
    "btlbf_mibf_set_scratch": (C.c_int, [_P, C.c_uint64]),
    "btlbf_mibf_insert_ids_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), _P, C.c_int, _P]),
    "btlbf_mibf_saturate_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), _P, C.c_int, _P, C.c_int, _P]),
    "btlbf_mibf_query_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), C.c_uint, _P, _P, _P, _P, C.c_int, _P]),
    "btlbf_mibf_classify_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), C.POINTER(MibfClassifyParams), _P, _P,
                                           C.c_uint64, _P, _P, _P, _P, C.c_int, _P]),
    "btlbf_mibf_classify_pairs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), C.POINTER(MibfClassifyParams), _P, _P,
                                            C.c_uint64, _P, _P, _P, _P, C.c_int, _P]),
    "btlbf_mibf_classify_paths": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "btlbf_mibf_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "btlbf_mibf_frame_probs": (C.c_int, [_P, C.c_uint, _P, C.c_uint64, C.POINTER(C.c_double)]),
    "btlbf_mibf_prob_single_frame": (C.c_double, [C.c_double, C.c_uint, C.c_double, C.c_uint]),
    "btlbf_interleave_mates": (C.c_int, [_P, _P, _P, _P, C.c_uint64, _P, _P, C.c_int, C.c_int, _P]),
    "btlbf_mibf_classify_tally": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint64, _P, _P, _P, C.c_int,
                                            C.c_int, _P]),
    "btlbf_mibf_classify_fastx_open": (C.c_int, [C.POINTER(_P), _P, C.c_char_p, C.c_char_p, C.c_uint32,
                                                 C.POINTER(MibfClassifyParams), _P, _P, C.c_uint64, C.c_uint64]),
    "btlbf_mibf_classify_fastx_next": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_P),
                                                 C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "btlbf_mibf_classify_fastx_tally": (C.c_int, [_P, _P, _P, _P]),
    "btlbf_mibf_classify_fastx_close": (None, [_P]),
    "btlbf_mibf_classify_fastx": (C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(MibfClassifyParams), _P, _P,
                                            C.c_uint64, C.c_uint64, _P, _P, _P, C.POINTER(FastxStats)]),
    "btlbf_mibf_build_fastx": (C.c_int, [C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_char_p), C.c_uint,
                                         C.POINTER(MibfBuildParams), C.POINTER(MibfBuildReport), C.POINTER(C.c_uint64)]),
    "btlbf_mibf_optimal_size": (C.c_uint64, [C.c_uint64, C.c_uint, C.c_double]),
    "btlbf_count_windows_seqs": (C.c_int, [C.c_uint, _P, C.c_uint64, C.POINTER(Layout), _P, C.c_int, C.c_int, _P]),
    "btlbf_count_windows_fastx": (C.c_int, [C.c_char_p, C.c_uint, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(FastxStats)]),
    "btlbf_mibf_id_counts": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "btlbf_mibf_download": (C.c_int, [_P, _P]),
    "btlbf_mibf_upload": (C.c_int, [_P, _P]),
    "btlbf_mibf_download_counts": (C.c_int, [_P, _P]),
    "btlbf_mibf_store": (C.c_int, [_P, C.c_char_p]),
    "btlbf_mibf_load": (C.c_int, [C.POINTER(_P), C.c_char_p, _P, C.c_uint]),
    "btlbf_insert_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), C.c_int, C.c_int, C.c_int, _P]),
    "btlbf_contains_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), _P, _P, _P, C.c_int, _P]),
    "btlbf_insert_and_check_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), _P, _P, _P, C.c_int, _P]),
    "btlbf_min_count_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), _P, _P, C.c_int, _P]),
    "btlbf_min_count_seqs_wide": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), _P, _P, C.c_int, _P]),
    "btlbf_min_count_hashes_wide": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_int, _P]),
    "btlbf_insert_hashes": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_int, C.c_int, _P]),
    "btlbf_contains_hashes": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_int, _P]),
    "btlbf_insert_and_check_hashes": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_int, C.c_int, _P]),
    "btlbf_min_count_hashes": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_int, _P]),
    "btlbf_insert_kmers": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_int, C.c_int, _P]),
    "btlbf_contains_kmers": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_int, _P]),
    "btlbf_hash_kmers": (C.c_int, [C.c_uint, C.c_uint, _P, C.c_uint64, _P, _P, C.c_int, C.c_int, _P]),
    "btlbf_hash_seqs": (C.c_int, [C.c_uint, C.c_uint, C.POINTER(C.c_char_p), C.c_uint, C.c_uint, _P, C.c_uint64,
                                  C.POINTER(Layout), _P, _P, _P, C.c_int, C.c_int, _P]),
    "btlbf_popcount": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "btlbf_filtered_popcount": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "btlbf_positions_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), C.c_uint, _P, _P, C.c_uint64, _P, _P,
                                       _P]),
    "btlbf_route_plan": (C.c_int, [_P, C.c_uint64, C.POINTER(Layout), C.c_uint, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64)]),
    "btlbf_route_windows": (C.c_int, [_P, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "btlbf_plan_read_grid": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_uint32)]),
    "btlbf_plan_pass_a": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_uint32)]),
    "btlbf_plan_spaced_lds": (C.c_int, [C.c_uint, C.POINTER(C.c_char_p), C.c_uint, C.c_uint, C.POINTER(C.c_uint32)]),
    "btlbf_route_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), C.c_uint64, C.c_uint, C.c_uint, C.c_int, _P, _P,
                                   _P, _P, _P, _P, C.c_uint64, _P, _P]),
    "btlbf_route_geometry": (C.c_int, [_P, C.c_uint64, C.POINTER(Layout), C.c_uint, C.c_uint, C.POINTER(C.c_uint32)]),
    "btlbf_owner_scratch_bytes": (C.c_int, [_P, C.c_uint64, C.POINTER(Layout), C.c_uint, C.c_uint, C.POINTER(C.c_uint64)]),
    "btlbf_apply_routed_bins": (C.c_int, [_P, _P, _P, C.c_uint, C.c_uint, C.c_uint, C.c_uint64, C.POINTER(Layout),
                                          C.c_uint, C.c_int, _P, C.c_uint64, _P, _P]),
    "btlbf_apply_routed": (C.c_int, [_P, _P, _P, C.c_uint, C.c_uint64, C.POINTER(Layout), C.c_uint, C.c_int, _P,
                                     C.c_uint64, _P, _P]),
    "btlbf_apply_spill": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P, C.c_uint64, _P, _P]),
    "btlbf_resolve_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), _P, C.c_uint64, _P, _P]),
    "btlbf_popcount_bits": (C.c_int, [_P, C.c_uint64, C.POINTER(C.c_uint64), C.c_int, _P]),
    "btlbf_insert_positions": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "btlbf_test_positions": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "btlbf_and_answers": (C.c_int, [_P, _P, C.c_uint64, C.c_uint, _P, C.c_int, _P]),
    "btlbf_synth_reads": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, C.c_int, _P]),
    "btlbf_microbench": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "btlbf_count_per_seq": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), C.c_uint, _P, _P, C.c_int, C.c_int, _P]),
    "btlbf_fastx_open": (C.c_int, [C.POINTER(_P), C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64]),
    "btlbf_fastx_open_range": (C.c_int, [C.POINTER(_P), C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int,
                                         C.c_uint64, C.c_uint64]),
    "btlbf_fastx_next": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64), C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "btlbf_fastx_records": (C.c_uint64, [_P]),
    "btlbf_fastx_close": (None, [_P]),
    "btlbf_insert_fastx": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.c_uint64, C.POINTER(FastxStats)]),
    "btlbf_contains_fastx": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.c_uint64, C.POINTER(FastxStats)]),
    "btlbf_screen_seqs": (C.c_int, [_P, C.c_uint, _P, C.c_uint64, C.POINTER(Layout), C.POINTER(ScreenParams), _P, _P, _P,
                                    C.c_int, _P]),
    "btlbf_screen_tally": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint, _P, _P, _P, C.c_int, C.c_int, _P]),
    "btlbf_screen_fastx_open": (C.c_int, [C.POINTER(_P), _P, C.c_uint, C.c_char_p, C.c_uint32, C.POINTER(ScreenParams),
                                          C.c_uint64]),
    "btlbf_screen_fastx_next": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_P), C.POINTER(_P),
                                          C.POINTER(_P)]),
    "btlbf_screen_fastx_tally": (C.c_int, [_P, _P, _P, _P]),
    "btlbf_screen_fastx_close": (None, [_P]),
    "btlbf_screen_fastx": (C.c_int, [_P, C.c_uint, C.c_char_p, C.c_uint32, C.POINTER(ScreenParams), C.c_uint64, _P, _P, _P,
                                     C.POINTER(FastxStats)]),
    "btlbf_card_create": (C.c_int, [C.POINTER(_P), C.c_uint, C.c_uint, C.c_uint, C.c_int]),
    "btlbf_card_destroy": (None, [_P]),
    "btlbf_card_clear": (C.c_int, [_P]),
    "btlbf_card_add_seqs": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Layout), C.c_int, _P]),
    "btlbf_card_add_fastx": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.c_uint64, C.POINTER(FastxStats)]),
    "btlbf_card_merge": (C.c_int, [_P, _P]),
    "btlbf_card_download": (C.c_int, [_P, _P, _P]),
    "btlbf_card_upload": (C.c_int, [_P, _P, _P]),
    "btlbf_card_histogram": (C.c_int, [_P, _P, C.c_uint]),
    "btlbf_card_solve": (C.c_int, [_P, C.c_uint, C.c_uint, C.c_uint, C.POINTER(CardEstimate), _P]),
    "btlbf_card_estimate_now": (C.c_int, [_P, C.c_uint, C.POINTER(CardEstimate), _P]),
}
EXPORTS = sorted(_PROTOS)


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7 (same SONAME as /opt/rocm's).  A process
    must run ONE HIP runtime: whichever copy is loaded first wins, and torch cannot see the GPU through
    the system copy.  So if torch is installed, load its copy before libbtlbf.so resolves the SONAME
    (without importing torch); a later `import torch` then finds its own runtime already in place."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load(path=LIB_PATH):
    """Load libbtlbf.so (no GPU needed to load).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(
            "%s not found: build it with `python -m btl_bloomfilter_amd.build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    _preload_torch_hip_runtime()
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != OK:
        raise BtlbfError(rc, load().btlbf_last_error().decode("utf-8", "replace"))
