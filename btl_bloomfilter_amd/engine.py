"""Host-side mirror of the reference's filter classes over the C ABI (include/btlbf.h).

Method names follow the reference (insert / contains / insertAndCheck / storeFilter / getPop ...,
/root/reference/BloomFilter.hpp:46-381, CountingBloomFilter.hpp:27-111) with batch arguments:
sequence buffers (bytes / numpy uint8 / torch uint8 tensors on the GPU) or (n, h) uint64 hash rows.
Buffers that are torch CUDA tensors are passed as device pointers; everything else is host memory
that the library stages itself."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (BLOOM, COUNTING8, DEVICE, HOST, INCREMENT_ALL, INCREMENT_MIN, ORDER_PARALLEL,
                   ORDER_SERIAL, Layout, check)


def _is_torch_cuda(x):
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def _stream_ptr(stream, buf=None):
    """hipStream_t for a call.  stream=None with a torch CUDA buffer means torch's CURRENT stream on that
    device (the stream the buffer's producer and the output zero-fills are ordered on), not the legacy
    NULL stream, which torch's non-blocking side streams do not synchronise with."""
    if stream is None:
        if buf is not None and _is_torch_cuda(buf):
            import torch

            return C.c_void_p(torch.cuda.current_stream(buf.device).cuda_stream)
        return None
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))


class _Buf:
    """pointer + length + memory space of a caller buffer; keeps the backing object alive"""

    def __init__(self, x, dtype=np.uint8):
        if _is_torch_cuda(x):
            assert x.is_contiguous()
            self.keep = x
            self.ptr = C.c_void_p(x.data_ptr())
            self.nbytes = x.numel() * x.element_size()
            self.mem = DEVICE
        else:
            if isinstance(x, str):
                x = x.encode("latin-1")
            if isinstance(x, (bytes, bytearray, memoryview)):
                x = np.frombuffer(bytes(x), dtype=np.uint8)
            a = np.ascontiguousarray(x, dtype=dtype)
            self.keep = a
            self.ptr = C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)
            self.nbytes = a.nbytes
            self.mem = HOST


def _layout(starts, read_len, mem):
    if starts is None and not read_len:
        return None, None
    lay = Layout()
    keep = None
    if starts is not None:
        b = _Buf(starts, np.uint64)
        if b.mem != mem:
            raise ValueError("starts must live in the same memory space as the sequence buffer")
        keep = b
        lay.starts = b.ptr
        lay.n_seqs = b.nbytes // 8 - 1
        lay.read_len = 0
    else:
        lay.starts = None
        lay.n_seqs = 0
        lay.read_len = int(read_len)
    return lay, keep


def bits_to_bool(bits, n):
    """per-window bitmap (uint64 words, bit p&63 of word p>>6) -> bool array of n windows"""
    b = np.ascontiguousarray(bits).view(np.uint8)
    return np.unpackbits(b, bitorder="little")[:n].astype(bool)


def _words(n):
    return (n + 63) // 64


def _out(b, shape, dtype):
    """A zeroed output in the memory space of the input _Buf `b` -> (output, its c_void_p); (None, None) for an
    optional output that was not asked for (shape None).  Device input: a torch tensor on the input's device, of
    torch's same-width signed type where torch has no unsigned one (bitmaps and hashes are int64).  Host input: a
    numpy array of at least one element along its first axis, sliced back to the shape asked for."""
    if shape is None:
        return None, None
    shape = shape if isinstance(shape, tuple) else (int(shape),)
    if b.mem == DEVICE:
        import torch

        name = np.dtype(dtype).name
        t = torch.zeros(shape, dtype=getattr(torch, name if name == "uint8" else name.lstrip("u")),
                        device=b.keep.device)
        return t, C.c_void_p(t.data_ptr())
    a = np.zeros((max(shape[0], 1),) + shape[1:], dtype)
    return a[: shape[0]], C.c_void_p(a.ctypes.data)


_MODES = {"auto": 0, "direct": 1, "partitioned": 2}
_COMBINE = {"or": _lib.COMBINE_OR, "and": _lib.COMBINE_AND, "andnot": _lib.COMBINE_ANDNOT, "add": _lib.COMBINE_ADD,
            "max": _lib.COMBINE_MAX, "min": _lib.COMBINE_MIN}


def _mode(mode):
    return _MODES[mode] if isinstance(mode, str) else int(mode)


class _Owned:
    """a library handle in self._h that the call named by `_destroy` releases"""

    _destroy = "btlbf_destroy"

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Filter(_Owned):
    kind = BLOOM

    def __init__(self, handle):
        self._h = handle
        self._L = _lib.load()

    # -- lifetime --------------------------------------------------------------------------
    @classmethod
    def _create(cls, size, hash_num, kmer_size, threshold=0, device=0, kind=None):
        L = _lib.load()
        h = C.c_void_p()
        check(L.btlbf_create(C.byref(h), cls.kind if kind is None else kind, int(size), int(hash_num), int(kmer_size),
                             int(threshold), int(device)))
        return h

    @classmethod
    def _load(cls, path, threshold=0, device=0, kind=None):
        L = _lib.load()
        h = C.c_void_p()
        check(L.btlbf_load(C.byref(h), cls.kind if kind is None else kind, str(path).encode(), int(threshold),
                           int(device)))
        return h

    # -- attributes (reference getters) ------------------------------------------------------
    def getHashNum(self):
        return self._L.btlbf_hash_num(self._h)

    def getKmerSize(self):
        return self._L.btlbf_kmer_size(self._h)

    def sizeInBytes(self):
        return self._L.btlbf_size_bytes(self._h)

    def localBytes(self):
        return self._L.btlbf_local_bytes(self._h)

    def device_ptr(self):
        return self._L.btlbf_device_ptr(self._h)

    def header(self):
        n = C.c_size_t()
        buf = C.create_string_buffer(1024)
        check(self._L.btlbf_header(self._h, buf, 1024, C.byref(n)))
        return buf.raw[: n.value]

    def storeFilter(self, path):
        check(self._L.btlbf_store(self._h, str(path).encode()))

    def storeShard(self, path):
        check(self._L.btlbf_store_shard(self._h, str(path).encode()))

    def clear(self, stream=None):
        check(self._L.btlbf_clear(self._h, _stream_ptr(stream)))

    def download(self):
        out = np.zeros(self.localBytes(), np.uint8)
        check(self._L.btlbf_download(self._h, C.c_void_p(out.ctypes.data), 0, out.nbytes))
        return out

    def upload(self, body):
        a = np.ascontiguousarray(body, np.uint8)
        check(self._L.btlbf_upload(self._h, C.c_void_p(a.ctypes.data), 0, a.nbytes))

    def compare(self, other):
        """(positions that differ, positions where self > other, where self < other) against another filter
        of the same geometry, computed in HBM (btlbf_compare); positions are bits or counters of the filter's width"""
        out = (C.c_uint64 * 3)()
        check(self._L.btlbf_compare(self._h, other._h, out))
        return tuple(out)

    def digest(self):
        """(sum, xor) digest of the local array computed in HBM (btlbf_digest); shard digests combine by + and ^"""
        out = (C.c_uint64 * 2)()
        check(self._L.btlbf_digest(self._h, out))
        return int(out[0]), int(out[1])

    # -- filter algebra (btlbf_clone / btlbf_combine / btlbf_fold / btlbf_threshold_bits) ----------------
    def _derived(self, handle):
        """a filter of this one's class around a handle the library made from it"""
        f = object.__new__(type(self))
        f.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        _Filter.__init__(f, handle)
        return f

    def copy(self):
        """a second filter with the same geometry, settings and body, copied in HBM (btlbf_clone)"""
        h = C.c_void_p()
        check(self._L.btlbf_clone(C.byref(h), self._h))
        return self._derived(h)

    def combine(self, others, op):
        """self = self OP others[0] OP ... in one pass over HBM (btlbf_combine; op: a _lib.COMBINE_* or its name);
        returns the popcount of the result (set bits / non-zero counters)"""
        others = list(others)
        arr = (C.c_void_p * max(len(others), 1))(*[o._h for o in others])
        pop = C.c_uint64()
        check(self._L.btlbf_combine(self._h, arr, len(others), _COMBINE[op] if isinstance(op, str) else int(op),
                                    C.byref(pop)))
        return pop.value

    def fold(self, factor):
        """the filter of size / factor positions that the same data would have built (btlbf_fold): bit filters
        exactly; counting filters exactly for incrementAll, as an upper bound for incrementMin"""
        h = C.c_void_p()
        check(self._L.btlbf_fold(C.byref(h), self._h, int(factor)))
        return self._derived(h)

    def setInsertMode(self, mode, scratch_bytes=0):
        """'auto' | 'direct' | 'partitioned' (see btlbf_set_insert_mode)"""
        check(self._L.btlbf_set_insert_mode(self._h, _mode(mode), int(scratch_bytes)))

    def releaseScratch(self):
        check(self._L.btlbf_release_scratch(self._h))

    def setProfiling(self, on=True):
        check(self._L.btlbf_set_profiling(self._h, int(bool(on))))

    def getProfile(self, reset=True):
        """{kernel slot name: (milliseconds, launches)} measured with HIP events on the launch stream"""
        ms = (C.c_double * _lib.PROF_SLOTS)()
        calls = (C.c_uint * _lib.PROF_SLOTS)()
        check(self._L.btlbf_get_profile(self._h, ms, calls, int(bool(reset))))
        return {n: (ms[i], calls[i]) for i, n in enumerate(_lib.PROF_NAMES) if calls[i]}

    def setQueryMode(self, mode):
        """'auto' | 'direct' | 'partitioned' (see btlbf_set_query_mode)"""
        check(self._L.btlbf_set_query_mode(self._h, _mode(mode)))

    # -- FASTA / FASTQ files (btlbf_insert_fastx / btlbf_contains_fastx) -----------------------------
    def insertFile(self, path, per_line=False, batch_bytes=0):
        """Insert every k-mer of a FASTA / FASTQ / one-sequence-per-line file (optionally gzipped).
        per_line=True treats every sequence line as its own sequence (the reference's loadBf);
        the default concatenates the lines of a FASTA record (contigsToBloom).  Returns the stats dict."""
        st = _lib.FastxStats()
        check(self._L.btlbf_insert_fastx(self._h, str(path).encode(), 1 if per_line else 0, int(batch_bytes),
                                         C.byref(st)))
        return st.as_dict()

    def containsFile(self, path, per_line=False, batch_bytes=0):
        """Query every k-mer of a file; stats['n_windows'] clean windows, stats['n_hits'] of them found."""
        st = _lib.FastxStats()
        check(self._L.btlbf_contains_fastx(self._h, str(path).encode(), 1 if per_line else 0, int(batch_bytes),
                                           C.byref(st)))
        return st.as_dict()

    def setSpacedSeeds(self, seeds, h2=1):
        arr = (C.c_char_p * len(seeds))(*[s.encode() if isinstance(s, str) else s for s in seeds])
        check(self._L.btlbf_set_spaced_seeds(self._h, arr, len(seeds), h2))

    # -- sequence buffers ----------------------------------------------------------------------
    def _query(self, fn, seq, starts, read_len, want_valid, want_counts, stream):
        b = _Buf(seq)
        lay, keep = _layout(starts, read_len, b.mem)
        n = b.nbytes
        hit, p_hit = _out(b, _words(n), np.uint64)
        valid, p_valid = _out(b, _words(n) if want_valid else None, np.uint64)
        cnt, p_cnt = _out(b, 2 if want_counts else None, np.uint64)
        check(fn(self._h, b.ptr, n, C.byref(lay) if lay else None, p_hit, p_valid, p_cnt, b.mem,
                 _stream_ptr(stream, b.keep)))
        return hit, valid, cnt

    def containsSeqs(self, seq, starts=None, read_len=0, want_valid=True, want_counts=False, stream=None):
        """contains() of every window of a sequence buffer -> (hit_bits, valid_bits, counts)"""
        return self._query(self._L.btlbf_contains_seqs, seq, starts, read_len, want_valid, want_counts, stream)

    def _insert_seqs(self, seq, starts, read_len, op, order, stream):
        b = _Buf(seq)
        lay, keep = _layout(starts, read_len, b.mem)
        check(self._L.btlbf_insert_seqs(self._h, b.ptr, b.nbytes, C.byref(lay) if lay else None, op, order,
                                        b.mem, _stream_ptr(stream, b.keep)))

    # -- hash rows -----------------------------------------------------------------------------
    def _rows(self, hashes):
        h = self.getHashNum()
        if _is_torch_cuda(hashes):
            b = _Buf(hashes)
            return b, b.nbytes // (8 * h)
        a = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, h)
        return _Buf(a, np.uint64), a.shape[0]

    def _rows_out(self, fn, hashes, *extra, stream=None, dtype=np.uint8):
        b, n = self._rows(hashes)
        out, optr = _out(b, n, dtype)
        check(fn(self._h, b.ptr, n, optr, *extra, b.mem, _stream_ptr(stream, b.keep)))
        return out


class BloomFilter(_Filter):
    """bit-array filter (reference: /root/reference/BloomFilter.hpp)"""

    kind = BLOOM

    def __init__(self, filterSize=None, hashNum=None, kmerSize=None, path=None, device=0, _handle=None):
        if _handle is not None:
            super().__init__(_handle)
        elif path is not None:
            super().__init__(self._load(path, 0, device))
        else:
            super().__init__(self._create(filterSize, hashNum, kmerSize, 0, device))

    @classmethod
    def shard(cls, global_bits, shard_index, shard_count, hashNum, kmerSize, device=0):
        L = _lib.load()
        h = C.c_void_p()
        check(L.btlbf_create_shard(C.byref(h), BLOOM, global_bits, shard_index, shard_count, hashNum, kmerSize,
                                   0, device))
        return cls(_handle=h)

    def getFilterSize(self):
        return self._L.btlbf_size(self._h)

    def getnEntry(self):
        return self._L.btlbf_get_n_entry(self._h)

    def gettEntry(self):
        return self._L.btlbf_get_t_entry(self._h)

    def setnEntry(self, v):
        self._L.btlbf_set_n_entry(self._h, v)

    def settEntry(self, v):
        self._L.btlbf_set_t_entry(self._h, v)

    def getPop(self):
        out = C.c_uint64()
        check(self._L.btlbf_popcount(self._h, C.byref(out)))
        return out.value

    def getFPR(self):
        return (self.getPop() / self.getFilterSize()) ** self.getHashNum()  # BloomFilter.hpp:346-350

    # batch forms of insert / contains / insertAndCheck over hash rows
    def insert(self, hashes, stream=None):
        b, n = self._rows(hashes)
        check(self._L.btlbf_insert_hashes(self._h, b.ptr, n, 0, ORDER_PARALLEL, b.mem, _stream_ptr(stream, b.keep)))

    def contains(self, hashes, stream=None):
        return self._rows_out(self._L.btlbf_contains_hashes, hashes, stream=stream)

    def insertAndCheck(self, hashes, serial=True, stream=None):
        return self._rows_out(self._L.btlbf_insert_and_check_hashes, hashes,
                              ORDER_SERIAL if serial else ORDER_PARALLEL, stream=stream)

    # insertSeq (BloomFilterUtil.h:10) over whole buffers
    def insertSeqs(self, seq, starts=None, read_len=0, stream=None):
        self._insert_seqs(seq, starts, read_len, 0, ORDER_PARALLEL, stream)

    def insertAndCheckSeqs(self, seq, starts=None, read_len=0, want_valid=True, want_counts=False, stream=None):
        return self._query(self._L.btlbf_insert_and_check_seqs, seq, starts, read_len, want_valid, want_counts,
                           stream)

    # set operations with filters of the same geometry, in place (each is one pass whatever the number of operands)
    def union(self, *others):
        self.combine(others, _lib.COMBINE_OR)
        return self

    def intersect(self, *others):
        self.combine(others, _lib.COMBINE_AND)
        return self

    def subtract(self, *others):
        self.combine(others, _lib.COMBINE_ANDNOT)
        return self

    __ior__ = union
    __iand__ = intersect
    __isub__ = subtract

    def __or__(self, other):
        return self.copy().union(other)

    def __and__(self, other):
        return self.copy().intersect(other)

    def __sub__(self, other):
        return self.copy().subtract(other)

    def microbench(self, kind, n_access):
        done = C.c_uint64()
        sec = C.c_double()
        check(self._L.btlbf_microbench(self._h, kind, n_access, C.byref(done), C.byref(sec)))
        return done.value, sec.value


class KmerBloomFilter(BloomFilter):
    """The surface the reference's SWIG module exposes as `BloomFilter` (swig/BloomFilter.i:17-59 =
    KmerBloomFilter.hpp:17-75): insert / contains take either a k-mer string or a row of precomputed
    hashes; together with insertSeq() below this replaces both the SWIG/Perl binding and the stale
    Boost.Python module under pythonInterface/.  K-mer strings are hashed on the GPU with the values of the
    reference's raw-k-mer path, NTC64(kmerSeq, k) -- which are not the iterator's for k % 4 == 0 and for
    k-mers with U (btlbf_insert_kmers in include/btlbf.h has the details)."""

    @staticmethod
    def _is_kmer(x):
        return isinstance(x, (str, bytes, bytearray))

    def _kmers(self, x):
        """one k-mer string, or a list of them -> (uint8 buffer of n*k bytes, n)"""
        k = self.getKmerSize()
        items = [x] if self._is_kmer(x) else list(x)
        out = bytearray()
        for it in items:
            b = it.encode("latin-1") if isinstance(it, str) else bytes(it)
            if len(b) < k:
                raise ValueError("k-mer shorter than kmerSize")
            out += b[:k]
        return np.frombuffer(bytes(out), np.uint8), len(items)

    def _kmer_buf(self, kmers):
        """strings, or a uint8 buffer of n*k bytes (numpy / torch on the GPU) -> (_Buf, n)"""
        if isinstance(kmers, np.ndarray) or _is_torch_cuda(kmers):
            b = _Buf(kmers)
            return b, b.nbytes // self.getKmerSize()
        buf, n = self._kmers(kmers)
        return _Buf(buf), n

    def insertKmers(self, kmers, stream=None):
        """KmerBloomFilter::insert(const char*) for a batch of raw k-mers (strings, or a uint8 buffer of n*k)"""
        b, n = self._kmer_buf(kmers)
        check(self._L.btlbf_insert_kmers(self._h, b.ptr, n, 0, ORDER_PARALLEL, b.mem, _stream_ptr(stream, b.keep)))

    def containsKmers(self, kmers, stream=None):
        """KmerBloomFilter::contains(const char*) for a batch of raw k-mers -> uint8 array"""
        b, n = self._kmer_buf(kmers)
        out, optr = _out(b, n, np.uint8)
        check(self._L.btlbf_contains_kmers(self._h, b.ptr, n, optr, b.mem, _stream_ptr(stream, b.keep)))
        return out

    def insert(self, x, stream=None):
        if self._is_kmer(x):
            return self.insertKmers(x, stream=stream)
        return super().insert(x, stream=stream)

    def contains(self, x, stream=None):
        if self._is_kmer(x):
            return bool(self.containsKmers(x, stream=stream)[0])
        r = super().contains(x, stream=stream)
        return bool(r[0]) if np.ndim(x) == 1 else r


def body_digest(body, first_word=0):
    """btlbf_digest restated with numpy over a host copy of a filter body (bytes / uint8 array): the definition in
    include/btlbf.h, for checking a digest against bytes that are at hand"""
    b = np.frombuffer(bytes(body), np.uint8) if not isinstance(body, np.ndarray) else body.view(np.uint8).ravel()
    if b.size % 8:
        b = np.concatenate([b, np.zeros(8 - b.size % 8, np.uint8)])
    w = b.view("<u8")
    nz = np.flatnonzero(w)

    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    with np.errstate(over="ignore"):
        m = mix(nz.astype(np.uint64) + np.uint64(first_word + 1)) | np.uint64(1)
        s = int((w[nz] * m).sum(dtype=np.uint64)) if nz.size else 0
        x = int(np.bitwise_xor.reduce(mix(w[nz] ^ m))) if nz.size else 0
    return s, x


def hash_kmers(kmers, h, k, device=0):
    """NTC64(kmerSeq, k) + NTE64 of raw k-mers (KmerBloomFilter's path; bytes of n*k) -> (hashes[n, h], valid[n])"""
    b = _Buf(kmers)
    n = b.nbytes // k
    hv = np.zeros((max(n, 1), h), np.uint64)
    ok = np.zeros(max(n, 1), np.uint8)
    if b.mem != HOST:
        raise ValueError("hash_kmers takes host buffers")
    check(_lib.load().btlbf_hash_kmers(k, h, b.ptr, n, C.c_void_p(hv.ctypes.data), C.c_void_p(ok.ctypes.data), HOST,
                                       device, None))
    return hv[:n], ok[:n]


def insertSeq(bloom, seq, numHashes=None, k=None):
    """insertSeq(KmerBloomFilter&, const string&, numHashes, k) of BloomFilterUtil.h:9-17 /
    swig/BloomFilter.i:59: every k-mer of `seq` in one fused launch.  numHashes / k must be the filter's
    own (the reference hashes with the arguments and inserts with the filter's hash count)."""
    if numHashes is not None and numHashes != bloom.getHashNum() or k is not None and k != bloom.getKmerSize():
        raise ValueError("insertSeq: numHashes / k differ from the filter's")
    s = seq.encode() if isinstance(seq, str) else bytes(seq)
    bloom.insertSeqs(np.frombuffer(s, np.uint8))


class CountingBloomFilter(_Filter):
    """counting filter (reference: CountingBloomFilter.hpp, CountingBloomFilter<T>): counter_bits = 8 (T = uint8_t, the
    default), 16, 32 or 64.  The wide kinds take the direct path only (include/btlbf.h); minimum counts and
    counters() come in the counter's dtype."""

    kind = COUNTING8

    def __init__(self, sizeInBytes=None, hashNum=None, kmerSize=None, countThreshold=0, path=None, device=0,
                 counter_bits=8):
        if counter_bits not in _lib.COUNTING_KIND:
            raise ValueError("counter_bits must be 8, 16, 32 or 64")
        kind = _lib.COUNTING_KIND[counter_bits]
        self.counter_bits = counter_bits
        self.dtype = np.dtype("<u%d" % (counter_bits // 8))
        if path is not None:
            super().__init__(self._load(path, countThreshold, device, kind))
        else:
            super().__init__(self._create(sizeInBytes, hashNum, kmerSize, countThreshold, device, kind))

    def counterBytes(self):
        return self._L.btlbf_counter_bytes(self._h)

    def counters(self):
        """the downloaded body viewed in the counter's dtype: size() counters"""
        return self.download().view(self.dtype)

    def size(self):
        return self._L.btlbf_size(self._h)

    def threshold(self):
        return self._L.btlbf_threshold(self._h)

    def popCount(self):
        out = C.c_uint64()
        check(self._L.btlbf_popcount(self._h, C.byref(out)))
        return out.value

    def filtered_popcount(self):
        out = C.c_uint64()
        check(self._L.btlbf_filtered_popcount(self._h, C.byref(out)))
        return out.value

    def FPR(self):
        return (self.popCount() / self.size()) ** self.getHashNum()

    def filtered_FPR(self):
        return (self.filtered_popcount() / self.size()) ** self.getHashNum()

    def merge(self, *others, op="add"):
        """self = self OP others, counter by counter, in place: "add" saturates at the counter's maximum (what
        incrementAll of all the inputs into one filter leaves), "max", "min".  Returns self."""
        if op not in ("add", "max", "min"):
            raise ValueError("merge: op must be 'add', 'max' or 'min'")
        self.combine(others, op)
        return self

    def toBloomFilter(self, threshold=None):
        """the BloomFilter of size() bits with bit p = (counter p >= threshold) (default: the filter's own threshold): its
        contains() is this filter's at that threshold, in 1/8 to 1/64 of the memory (btlbf_threshold_bits)"""
        h = C.c_void_p()
        check(self._L.btlbf_threshold_bits(C.byref(h), self._h, 0 if threshold is None else int(threshold)))
        return BloomFilter(_handle=h)

    def insert(self, hashes, serial=False, stream=None):  # = incrementMin (CountingBloomFilter.hpp:198-204)
        self.incrementMin(hashes, serial, stream)

    def incrementMin(self, hashes, serial=False, stream=None):
        b, n = self._rows(hashes)
        check(self._L.btlbf_insert_hashes(self._h, b.ptr, n, INCREMENT_MIN,
                                          ORDER_SERIAL if serial else ORDER_PARALLEL, b.mem,
                                          _stream_ptr(stream, b.keep)))

    def incrementAll(self, hashes, serial=False, stream=None):
        b, n = self._rows(hashes)
        check(self._L.btlbf_insert_hashes(self._h, b.ptr, n, INCREMENT_ALL,
                                          ORDER_SERIAL if serial else ORDER_PARALLEL, b.mem,
                                          _stream_ptr(stream, b.keep)))

    def minCount(self, hashes, stream=None):
        if self.counter_bits == 8:
            return self._rows_out(self._L.btlbf_min_count_hashes, hashes, stream=stream)
        return self._rows_out(self._L.btlbf_min_count_hashes_wide, hashes, stream=stream, dtype=self.dtype)

    def contains(self, hashes, stream=None):
        return self._rows_out(self._L.btlbf_contains_hashes, hashes, stream=stream)

    def insertAndCheck(self, hashes, serial=True, stream=None):
        return self._rows_out(self._L.btlbf_insert_and_check_hashes, hashes,
                              ORDER_SERIAL if serial else ORDER_PARALLEL, stream=stream)

    def insertSeqs(self, seq, starts=None, read_len=0, increment_all=False, serial=False, stream=None):
        self._insert_seqs(seq, starts, read_len, INCREMENT_ALL if increment_all else INCREMENT_MIN,
                          ORDER_SERIAL if serial else ORDER_PARALLEL, stream)

    def minCountSeqs(self, seq, starts=None, read_len=0, stream=None):
        b = _Buf(seq)
        lay, keep = _layout(starts, read_len, b.mem)
        n = b.nbytes
        mn, p1 = _out(b, n, self.dtype)
        valid, p2 = _out(b, _words(n), np.uint64)
        fn = self._L.btlbf_min_count_seqs if self.counter_bits == 8 else self._L.btlbf_min_count_seqs_wide
        check(fn(self._h, b.ptr, n, C.byref(lay) if lay else None, p1, p2, b.mem, _stream_ptr(stream, b.keep)))
        return mn, valid

    # raw k-mers (btlbf_insert_kmers / btlbf_contains_kmers): n k-mers of kmerSize bytes each, back to back
    def insertKmers(self, kmers, increment_all=False, serial=False, stream=None):
        b = _Buf(kmers)
        check(self._L.btlbf_insert_kmers(self._h, b.ptr, b.nbytes // self.getKmerSize(),
                                         INCREMENT_ALL if increment_all else INCREMENT_MIN,
                                         ORDER_SERIAL if serial else ORDER_PARALLEL, b.mem, _stream_ptr(stream, b.keep)))

    def containsKmers(self, kmers, stream=None):
        b = _Buf(kmers)
        n = b.nbytes // self.getKmerSize()
        out, optr = _out(b, n, np.uint8)
        check(self._L.btlbf_contains_kmers(self._h, b.ptr, n, optr, b.mem, _stream_ptr(stream, b.keep)))
        return out


class RankSupport(_Owned):
    """sdsl::bit_vector_il<512> + rank_support_il<1> over a bit filter, in HBM (btlbf_rank_*): what the
    reference's miBF uses to turn a set bit into an index of its ID array (MIBloomFilter.hpp:527,801-803)"""

    _destroy = "btlbf_rank_destroy"

    def __init__(self, bloom):
        self._L = _lib.load()
        h = C.c_void_p()
        check(self._L.btlbf_rank_create(C.byref(h), bloom._h))
        self._h = h

    def ones(self):
        return self._L.btlbf_rank_ones(self._h)

    def interleaved(self):
        """the interleaved vector as (n_blocks, 9) uint64: column 0 = set bits before the block"""
        out = np.zeros(self._L.btlbf_rank_words(self._h), np.uint64)
        check(self._L.btlbf_rank_download(self._h, C.c_void_p(out.ctypes.data)))
        return out.reshape(-1, 9)

    def rank(self, values, hashes=False):
        """(rank, bit) of positions, or of hash values reduced modulo the filter size (getRankPos)"""
        v = np.ascontiguousarray(values, np.uint64).ravel()
        r = np.zeros(max(v.size, 1), np.uint64)
        b = np.zeros(max(v.size, 1), np.uint8)
        check(self._L.btlbf_rank_query(self._h, C.c_void_p(v.ctypes.data), v.size, int(bool(hashes)),
                                       C.c_void_p(r.ctypes.data), C.c_void_p(b.ctypes.data), HOST, None))
        return r[: v.size], b[: v.size]


def _hash_seqs(seq, k, h, seeds, h2, starts, read_len, device, stream):
    L = _lib.load()
    b = _Buf(seq)
    lay, keep = _layout(starts, read_len, b.mem)
    n = b.nbytes
    sarr = None
    ns = 0
    if seeds is not None:
        ns = len(seeds)
        sarr = (C.c_char_p * ns)(*[s.encode() if isinstance(s, str) else s for s in seeds])
    hv, p_hv = _out(b, (n, h), np.uint64)
    valid, p_valid = _out(b, _words(n), np.uint64)
    st, p_st = _out(b, n if seeds is not None else None, np.uint64)
    check(L.btlbf_hash_seqs(k, h, sarr, ns, h2, b.ptr, n, C.byref(lay) if lay else None, p_hv, p_valid, p_st, b.mem,
                            device, _stream_ptr(stream, b.keep)))
    return hv, valid, st


def hash_seqs(seq, h, k, starts=None, read_len=0, device=0, stream=None):
    """ntHashIterator(seq, h, k) over a whole buffer (vendor/ntHashIterator.hpp:38):
    -> (hashes[n, h], valid_bits).  Window p is emitted by the iterator iff its valid bit is set."""
    hv, valid, _ = _hash_seqs(seq, k, h, None, 0, starts, read_len, device, stream)
    return hv, valid


def sthash_seqs(seq, seeds, h2, k, starts=None, read_len=0, device=0, stream=None):
    """stHashIterator(seq, parseSeed(seeds), len(seeds), h2, k) (vendor/stHashIterator.hpp:53):
    -> (hashes[n, len(seeds)*h2], valid_bits, strand_bits[n])"""
    return _hash_seqs(seq, k, len(seeds) * h2, seeds, h2, starts, read_len, device, stream)


def synth_reads_device(seed, first, n_reads, read_len, device=0, stream=None):
    """synthetic reads of SURVEY.md 8d generated in HBM -> torch uint8 tensor (n_reads*read_len)"""
    import torch

    out = torch.empty(n_reads * read_len, dtype=torch.uint8, device="cuda:%d" % device)
    check(_lib.load().btlbf_synth_reads(C.c_void_p(out.data_ptr()), seed, first, n_reads, read_len, device,
                                        _stream_ptr(stream, out)))
    return out


def count_per_seq(hit_bits, valid_bits, n_bytes, k, starts=None, read_len=0, device=0, stream=None):
    """per-sequence (hits, clean windows) from the per-window bitmaps of containsSeqs / insertAndCheckSeqs
    over a buffer of n_bytes bytes (btlbf_count_per_seq): what a read classifier needs per read"""
    hb = _Buf(hit_bits, np.uint64)
    lay, keep = _layout(starts, read_len, hb.mem)
    if lay is None:
        raise ValueError("count_per_seq needs starts or read_len")
    n_seqs = lay.n_seqs if starts is not None else n_bytes // read_len
    vb = _Buf(valid_bits, np.uint64) if valid_bits is not None else None
    hits, p1 = _out(hb, n_seqs, np.uint32)
    valid, p2 = _out(hb, n_seqs, np.uint32)
    check(_lib.load().btlbf_count_per_seq(hb.ptr, vb.ptr if vb is not None else None, int(n_bytes), C.byref(lay), int(k),
                                           p1, p2, hb.mem, device, _stream_ptr(stream, hb.keep)))
    return hits, valid


def countWindows(seq, k, starts=None, read_len=0, device=0, stream=None):
    """(windows, clean windows) of the sequences of a buffer (btlbf_count_windows_seqs): a window is k bytes inside one
    sequence, clean when the hash kernels accept every byte of it.  No hashing; host or device memory."""
    b = _Buf(seq)
    lay, keep = _layout(starts, read_len, b.mem)
    out, optr = _out(b, 2, np.uint64)
    dev = (b.keep.device.index or 0) if b.mem == DEVICE else device
    check(_lib.load().btlbf_count_windows_seqs(int(k), b.ptr, b.nbytes, C.byref(lay) if lay else None, optr, b.mem, dev,
                                                _stream_ptr(stream, b.keep)))
    if b.mem == DEVICE:
        out = out.cpu().numpy()
    return int(out[0]), int(out[1])


def countWindowsFile(path, k, per_line=False, batch_bytes=0, whole=False, device=0):
    """countWindows over a FASTA / FASTQ file (btlbf_count_windows_fastx) -> the call's statistics: n_windows = clean
    windows, n_hits = windows, n_records, n_bases, n_batches, seconds"""
    st = _lib.FastxStats()
    flags = (_lib.FASTX_LINES if per_line else 0) | (_lib.FASTX_WHOLE if whole else 0)
    check(_lib.load().btlbf_count_windows_fastx(str(path).encode(), int(k), flags, int(batch_bytes), int(device),
                                                 C.byref(st)))
    return st.as_dict()


def fastx_batches(path, k, per_line=False, batch_bytes=0, pageable=True, byte_range=None, fmt=None, whole=False):
    """Iterate over the parser's batches as (bases: bytes, starts: list[int]) -- the host-side reader
    behind insertFile (btlbf_fastx_open / btlbf_fastx_next); needs no GPU.  byte_range=(begin, end) with
    fmt in {"fasta", "fastq", "plain"}: only the records that start in that byte range of an
    uncompressed file (btlbf_fastx_open_range, the unit of parallel parsing).  whole: BTLBF_FASTX_WHOLE, no sequence is
    cut at a batch boundary (one longer than a batch is an error) and an empty FASTQ read is an empty sequence."""
    L = _lib.load()
    r = C.c_void_p()
    flags = (1 if per_line else 0) | (2 if pageable else 0) | (_lib.FASTX_WHOLE if whole else 0)
    if byte_range is None:
        check(L.btlbf_fastx_open(C.byref(r), str(path).encode(), flags, int(k), int(batch_bytes)))
    else:
        check(L.btlbf_fastx_open_range(C.byref(r), str(path).encode(), flags, int(k), int(batch_bytes),
                                       {"fasta": 1, "fastq": 2, "plain": 3}[fmt], int(byte_range[0]),
                                       int(byte_range[1])))
    try:
        while True:
            b, s = C.c_void_p(), C.c_void_p()
            nb, ns = C.c_uint64(), C.c_uint64()
            check(L.btlbf_fastx_next(r, C.byref(b), C.byref(nb), C.byref(s), C.byref(ns)))
            if ns.value == 0:
                return
            bases = C.string_at(b.value, nb.value) if nb.value else b""
            starts = list((C.c_uint64 * (ns.value + 1)).from_address(s.value))
            yield bases, starts
    finally:
        L.btlbf_fastx_close(r)


# btlbf_mibf_hit
HIT_DTYPE = np.dtype([("id", "<u4"), ("count", "<u2"), ("nonSatCount", "<u2"), ("totalCount", "<u2"),
                      ("totalNonSatCount", "<u2"), ("nonSatFrameCount", "<u2"), ("solidCount", "<u2")])


def hits_from_words(words):
    """[..., 4] 32-bit words of btlbf_mibf_hit records (host) -> structured array [...] of HIT_DTYPE"""
    w = np.ascontiguousarray(np.asarray(words).astype(np.uint32, copy=False))
    return w.view(HIT_DTYPE).reshape(w.shape[:-1])


def interleave_mates(reads1, reads2):
    """two lists of equal length (mate 1 and mate 2 of every pair; bytes, str or uint8 arrays) -> (buffer, starts): the
    host buffer mate 1, mate 2, mate 1, ... and its 2 * n_pairs + 1 offsets, as MIBloomFilter.classifyPairs takes them"""
    if len(reads1) != len(reads2):
        raise ValueError("interleave_mates: %d first mates, %d second mates" % (len(reads1), len(reads2)))
    as_u8 = lambda s: np.frombuffer(s.encode() if isinstance(s, str) else s, np.uint8) if isinstance(s, (str, bytes, bytearray)) \
        else np.ascontiguousarray(s, np.uint8)
    mates = [as_u8(s) for pair in zip(reads1, reads2) for s in pair]
    starts = np.zeros(len(mates) + 1, np.uint64)
    if mates:
        starts[1:] = np.cumsum([m.size for m in mates])
    return (np.concatenate(mates) if mates else np.zeros(0, np.uint8)), starts


def interleave_mates_device(seq1, starts1, seq2, starts2, stream=None):
    """interleave_mates on the GPU (btlbf_interleave_mates): two ragged buffers -- torch uint8 tensors of bases and int64
    tensors of n_pairs + 1 offsets on one device, any alignment -- -> (buffer, starts) as classifyPairs takes them"""
    import torch

    n_pairs = starts1.numel() - 1
    if starts2.numel() - 1 != n_pairs:
        raise ValueError("interleave_mates_device: %d first mates, %d second mates" % (n_pairs, starts2.numel() - 1))
    bufs = [seq1, seq2, starts1.contiguous(), starts2.contiguous()]
    if not all(_is_torch_cuda(x) for x in bufs) or not seq1.is_contiguous() or not seq2.is_contiguous():
        raise ValueError("interleave_mates_device takes contiguous tensors on the GPU")
    out = torch.empty(seq1.numel() + seq2.numel(), dtype=torch.uint8, device=seq1.device)
    out_starts = torch.empty(2 * n_pairs + 1, dtype=torch.int64, device=seq1.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(_lib.load().btlbf_interleave_mates(ptr(seq1), ptr(bufs[2]), ptr(seq2), ptr(bufs[3]), n_pairs, ptr(out),
                                             ptr(out_starts), DEVICE, seq1.device.index or 0, _stream_ptr(stream, seq1)))
    return out, out_starts


def classify_tally(hits, n_hits, sat_count, eval_count, n_ids, best=None, any_=None, totals=None, device=0, stream=None):
    """btlbf_mibf_classify_tally: adds the summary of one batch of classify results to (best[n_ids], any[n_ids],
    totals[6]) and returns them.  Host results (hits as HIT_DTYPE or 32-bit words) with uint64 numpy totals, or device
    results (classify's tensors) with int64 tensors; the totals are made, zeroed, where they are not given."""
    b = _Buf(hits.view(np.uint32) if isinstance(hits, np.ndarray) else hits, np.uint32)
    n_rows = len(n_hits)
    max_results = (b.nbytes // 16) // n_rows if n_rows else max(int(np.prod(hits.shape[1:2])), 1)
    outs = []
    for x, n in ((best, n_ids), (any_, n_ids), (totals, 6)):
        if x is None:
            x, _ = _out(b, n, np.uint64)
        outs.append(x)
    args = [_Buf(x, np.uint32) for x in (n_hits, sat_count, eval_count)] + \
        [_Buf(x, np.uint64) if b.mem == HOST else _Buf(x) for x in outs]
    if any(a.mem != b.mem for a in args):
        raise ValueError("classify_tally: all arrays live in one memory space")
    for x, a in zip(outs, args[3:]):
        if b.mem == HOST and a.keep is not x:
            raise ValueError("classify_tally: the totals are contiguous uint64 arrays")
    check(_lib.load().btlbf_mibf_classify_tally(b.ptr, args[0].ptr, args[1].ptr, args[2].ptr, n_rows, max(max_results, 1),
                                                int(n_ids), args[3].ptr, args[4].ptr, args[5].ptr, b.mem,
                                                (b.keep.device.index or 0) if b.mem == DEVICE else device,
                                                _stream_ptr(stream, b.keep)))
    return tuple(outs)


class MIBloomFilter(_Owned):
    """Multi-index Bloom filter over a stage-1 bit filter (btlbf_mibf_*; MIBloomFilter.hpp, MIBFConstructSupport.hpp,
    MIBFQuerySupport.hpp): an ID array of uint16 (id_bytes=2) or uint32 (id_bytes=4) in HBM, addressed by
    rank(hash % size).  The stage-1 filter may be closed once this object exists."""

    _destroy = "btlbf_mibf_destroy"

    def __init__(self, stage1_filter, id_bytes=2, _handle=None):
        self._L = _lib.load()
        self.id_bytes = int(id_bytes)
        self.dtype = np.uint16 if self.id_bytes == 2 else np.uint32
        if _handle is None:
            h = C.c_void_p()
            check(self._L.btlbf_mibf_create(C.byref(h), stage1_filter._h, self.id_bytes))
            _handle = h
        self._h = _handle
        self.mask = 1 << (8 * self.id_bytes - 1)

    @classmethod
    def load(cls, path, bloom, id_bytes=2):
        """MIBloomFilter(path) (MIBloomFilter.hpp:149-248); the bit vector comes from `bloom` (no .sdsl file)"""
        L = _lib.load()
        h = C.c_void_p()
        check(L.btlbf_mibf_load(C.byref(h), str(path).encode(), bloom._h, int(id_bytes)))
        return cls(None, id_bytes, _handle=h)

    @staticmethod
    def calcOptimalSize(entries, hash_num, occupancy):
        """calcOptimalSize (MIBloomFilter.hpp:84-88): bits for `entries` entries of hash_num values at that occupancy"""
        return _lib.load().btlbf_mibf_optimal_size(int(entries), int(hash_num), float(occupancy))

    @classmethod
    def buildFromFiles(cls, paths, k, h=None, seeds=None, id_bytes=2, bits=0, expected_entries=0, occupancy=0.5,
                       ids="file", first_id=1, saturation="parallel", per_line=False, batch_bytes=0, scratch_bytes=0,
                       device=0):
        """A miBF from FASTA / FASTQ files (plain or gzip), stages 1-4 in one call (btlbf_mibf_build_fastx): size the bit
        vector (bits, or calcOptimalSize of expected_entries, or of the files' clean windows, counted), insert every
        sequence into the stage-1 filter, insertIDs, insertSaturation.  ids: "file" (file j gets first_id + j) or "record"
        (record r over all files gets first_id + r); saturation: "parallel" (one parallel call per parser batch of
        batch_bytes), "serial" (the reference's order) or None.  Whole records only: batch_bytes (0: 64 MiB) must hold the
        longest.  -> (mibf, stage-1 BloomFilter, report dict; report["records_per_file"] lists the files' records)."""
        L = _lib.load()
        paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else list(paths)
        enc = [p if isinstance(p, bytes) else str(p).encode() for p in paths]
        parr = (C.c_char_p * max(len(enc), 1))(*enc)
        sarr = None
        if seeds is not None:
            sarr = (C.c_char_p * len(seeds))(*[x.encode() if isinstance(x, str) else x for x in seeds])
        par = _lib.MibfBuildParams(
            int(k), int(h) if h is not None else (len(seeds) if seeds is not None else 0), sarr,
            len(seeds) if seeds is not None else 0, int(id_bytes), int(bits), int(expected_entries), float(occupancy),
            {"file": _lib.MIBF_ID_PER_FILE, "record": _lib.MIBF_ID_PER_RECORD}[ids], int(first_id),
            {None: _lib.MIBF_SAT_NONE, "none": _lib.MIBF_SAT_NONE, "serial": _lib.MIBF_SAT_SERIAL,
             "parallel": _lib.MIBF_SAT_PARALLEL}[saturation],
            _lib.FASTX_LINES if per_line else 0, int(batch_bytes), int(scratch_bytes), int(device))
        rep = _lib.MibfBuildReport()
        per_file = (C.c_uint64 * max(len(enc), 1))()
        hm, hf = C.c_void_p(), C.c_void_p()
        check(L.btlbf_mibf_build_fastx(C.byref(hm), C.byref(hf), parr, len(enc), C.byref(par), C.byref(rep), per_file))
        report = rep.as_dict()
        report["records_per_file"] = list(per_file)[: len(enc)]
        return cls(None, id_bytes, _handle=hm), BloomFilter(_handle=hf), report

    def getPop(self):
        return self._L.btlbf_mibf_size(self._h)

    def size(self):
        return self._L.btlbf_mibf_bits(self._h)

    def getHashNum(self):
        return self._L.btlbf_mibf_hash_num(self._h)

    def getKmerSize(self):
        return self._L.btlbf_mibf_kmer_size(self._h)

    def setScratchBudget(self, nbytes):
        check(self._L.btlbf_mibf_set_scratch(self._h, int(nbytes)))

    def _seq_args(self, seqs, ids, starts, read_len):
        b = _Buf(seqs)
        lay, keep = _layout(starts, read_len, b.mem)
        if ids is None:
            return b, lay, keep, None
        if b.mem == DEVICE:
            import torch

            ib = _Buf(ids.to(torch.int32).contiguous() if ids.dtype != torch.int32 else ids.contiguous())
        else:
            ib = _Buf(np.ascontiguousarray(ids, np.uint32), np.uint32)
        return b, lay, keep, ib

    def insertIDs(self, seqs, ids, starts=None, read_len=0, stream=None):
        """insertMIBF (MIBFConstructSupport.hpp:109-130) of every sequence with its id, in sequence order"""
        b, lay, keep, ib = self._seq_args(seqs, ids, starts, read_len)
        check(self._L.btlbf_mibf_insert_ids_seqs(self._h, b.ptr, b.nbytes, C.byref(lay) if lay else None, ib.ptr, b.mem,
                                                 _stream_ptr(stream, b.keep)))

    def insertSaturation(self, seqs, ids, starts=None, read_len=0, serial=False, stream=None):
        """insertSaturation (MIBFConstructSupport.hpp:132-214) -> {clean, found, mutated, saturated}"""
        b, lay, keep, ib = self._seq_args(seqs, ids, starts, read_len)
        out, optr = _out(b, 4, np.uint64)
        check(self._L.btlbf_mibf_saturate_seqs(self._h, b.ptr, b.nbytes, C.byref(lay) if lay else None, ib.ptr,
                                               ORDER_SERIAL if serial else ORDER_PARALLEL, optr, b.mem,
                                               _stream_ptr(stream, b.keep)))
        if b.mem == DEVICE:
            out = out.cpu().numpy().astype(np.uint64)
        return dict(zip(("clean", "found", "mutated", "saturated"), (int(x) for x in out)))

    def query(self, seqs, max_miss=0, starts=None, read_len=0, want_counts=False, stream=None):
        """getMatchSignature (MIBFQuerySupport.hpp:158-217) of every window -> (values[n, h], match_bits, valid_bits)
        (+ counts {clean, matched} with want_counts); decode(values) gives (id, saturated)"""
        b, lay, keep, _ = self._seq_args(seqs, None, starts, read_len)
        n, h = b.nbytes, self.getHashNum()
        vals, p_vals = _out(b, (n, h), self.dtype)
        hit, p_hit = _out(b, _words(n), np.uint64)
        valid, p_valid = _out(b, _words(n), np.uint64)
        cnt, p_cnt = _out(b, 2, np.uint64)
        check(self._L.btlbf_mibf_query_seqs(self._h, b.ptr, n, C.byref(lay) if lay else None, int(max_miss), p_vals,
                                            p_hit, p_valid, p_cnt, b.mem, _stream_ptr(stream, b.keep)))
        return (vals, hit, valid, cnt) if want_counts else (vals, hit, valid)

    def classify(self, seqs, per_frame_prob, min_count, *, extra_count=1.0, extra_frame_limit=0, max_miss=0,
                 min_frames=1, best_hit_agree=False, max_results=8, starts=None, read_len=0, stream=None):
        """MIBFQuerySupport<T>::query(itr, minCount) (MIBFQuerySupport.hpp:95-109) of every sequence ->
        (hits[n_seqs, max_results] (HIT_DTYPE), n_hits[n_seqs], sat_count[n_seqs], eval_count[n_seqs]).
        per_frame_prob[id] and min_count[id] are the reference's perFrameProb and minCount vectors; extra_count,
        extra_frame_limit, max_miss, min_frames (its minCount constructor argument) and best_hit_agree its constructor
        arguments.  n_hits counts every significant result; the first max_results of them are in hits.  Device
        input: the tables and results are torch tensors on that device (hits as int32[n_seqs, max_results, 4]:
        hits_from_words decodes a host copy)."""
        return self._classify(self._L.btlbf_mibf_classify_seqs, 1, seqs, per_frame_prob, min_count, extra_count,
                              extra_frame_limit, max_miss, min_frames, best_hit_agree, max_results, starts, read_len, stream)

    def classifyPairs(self, seqs, per_frame_prob, min_count, *, extra_count=1.0, extra_frame_limit=0, max_miss=0,
                      min_frames=1, best_hit_agree=False, max_results=8, starts=None, read_len=0, stream=None):
        """MIBFQuerySupport<T>::query(itr1, itr2, minCount) (MIBFQuerySupport.hpp:111-130) of every read pair of an
        interleaved buffer: sequences 2i and 2i + 1 are mate 1 and mate 2 of pair i (interleave_mates builds such a
        buffer from two lists), their number must be even.  One walk per pair over the frames of both mates in turn,
        into one set of counters and with one early stop.  Arguments and results as for classify, one row per pair."""
        return self._classify(self._L.btlbf_mibf_classify_pairs, 2, seqs, per_frame_prob, min_count, extra_count,
                              extra_frame_limit, max_miss, min_frames, best_hit_agree, max_results, starts, read_len, stream)

    def _classify(self, fn, per_row, seqs, per_frame_prob, min_count, extra_count, extra_frame_limit, max_miss, min_frames,
                  best_hit_agree, max_results, starts, read_len, stream):
        """classify / classifyPairs: per_row sequences of the layout make one result row"""
        b = _Buf(seqs)
        lay, keep = _layout(starts, read_len, b.mem)
        if lay is None:
            raise ValueError("classify needs starts or read_len")
        n_seqs = (lay.n_seqs if starts is not None else b.nbytes // read_len) // per_row
        n_ids = len(per_frame_prob)
        if len(min_count) != n_ids:
            raise ValueError("per_frame_prob and min_count must have one entry per id")
        if b.mem == DEVICE:
            import torch

            prob = _Buf(torch.as_tensor(per_frame_prob, dtype=torch.float64, device=b.keep.device).contiguous())
            minc = _Buf(torch.as_tensor(min_count, dtype=torch.int32, device=b.keep.device).contiguous())
        else:
            prob = _Buf(np.ascontiguousarray(per_frame_prob, np.float64), np.float64)
            minc = _Buf(np.ascontiguousarray(min_count, np.uint32), np.uint32)
        par = _lib.MibfClassifyParams(float(extra_count), int(extra_frame_limit), int(max_miss), int(min_frames),
                                      int(bool(best_hit_agree)), int(max_results))
        words, p_hits = _out(b, (n_seqs, max(int(max_results), 1), 4), np.uint32)
        n_hits, p_n = _out(b, n_seqs, np.uint32)
        sat, p_sat = _out(b, n_seqs, np.uint32)
        ev, p_ev = _out(b, n_seqs, np.uint32)
        check(fn(self._h, b.ptr, b.nbytes, C.byref(lay), C.byref(par), prob.ptr, minc.ptr, n_ids, p_hits, p_n, p_sat, p_ev,
                 b.mem, _stream_ptr(stream, b.keep)))
        if b.mem == DEVICE:
            return words, n_hits, sat, ev
        return hits_from_words(words), n_hits, sat, ev

    def calcFrameProbs(self, n_ids, allowed_miss=0):
        """calcFrameProbs (MIBloomFilter.hpp:664-679) for a perFrameProb vector of n_ids entries -> (probs[n_ids],
        sat_prop).  probs[0] is not written by the reference and is 0 here."""
        probs = np.zeros(max(int(n_ids), 1), np.float64)
        sat = C.c_double()
        check(self._L.btlbf_mibf_frame_probs(self._h, int(allowed_miss), C.c_void_p(probs.ctypes.data), int(n_ids),
                                             C.byref(sat)))
        return probs[: int(n_ids)], sat.value

    @staticmethod
    def calcProbSingleFrame(occupancy, hash_num, freq, allowed_misses):
        """calcProbSingleFrame (MIBloomFilter.hpp:65-77)"""
        return _lib.load().btlbf_mibf_prob_single_frame(float(occupancy), int(hash_num), float(freq), int(allowed_misses))

    def classifyFile(self, path, per_frame_prob, min_count, *, path2=None, interleaved=False, batch_bytes=0,
                     summary_only=False, per_line=False, extra_count=1.0, extra_frame_limit=0, max_miss=0, min_frames=1,
                     best_hit_agree=False, max_results=8):
        """classify / classifyPairs of the reads of a FASTA / FASTQ file (plain or gzip), in file order
        (btlbf_mibf_classify_fastx_*): single reads; with path2, record i of both files as pair i; with interleaved,
        records 2i and 2i + 1 of the one file.  An iterator of (first_row, hits, n_hits, sat_count, eval_count) per batch
        of at most batch_bytes bases (0: 64 MiB): numpy arrays as classify returns them, copied out of the library's
        buffers; its tally() gives the running summary of the rows delivered so far, close() ends it early.  With
        summary_only=True no per-read result leaves the GPU and the call returns (best[n_ids], any[n_ids], totals):
        reads per id by their first result, by any of their first max_results results, and {rows, without a result,
        with several, with more than max_results, sum of satCount, sum of
        evalCount}.  The classify keywords are those of classify."""
        n_ids = len(per_frame_prob)
        if len(min_count) != n_ids:
            raise ValueError("per_frame_prob and min_count must have one entry per id")
        prob = np.ascontiguousarray(per_frame_prob, np.float64)
        minc = np.ascontiguousarray(min_count, np.uint32)
        par = _lib.MibfClassifyParams(float(extra_count), int(extra_frame_limit), int(max_miss), int(min_frames),
                                      int(bool(best_hit_agree)), int(max_results))
        flags = (_lib.FASTX_LINES if per_line else 0) | (_lib.CLASSIFY_INTERLEAVED if interleaved else 0)
        p1 = str(path).encode()
        p2 = str(path2).encode() if path2 is not None else None
        if summary_only:
            best, any_, totals = np.zeros(max(n_ids, 1), np.uint64), np.zeros(max(n_ids, 1), np.uint64), np.zeros(6, np.uint64)
            check(self._L.btlbf_mibf_classify_fastx(self._h, p1, p2, flags, C.byref(par), C.c_void_p(prob.ctypes.data),
                                                    C.c_void_p(minc.ctypes.data), n_ids, int(batch_bytes),
                                                    C.c_void_p(best.ctypes.data), C.c_void_p(any_.ctypes.data),
                                                    C.c_void_p(totals.ctypes.data), None))
            return best[:n_ids], any_[:n_ids], totals
        return _ClassifyFile(self, p1, p2, flags, par, prob, minc, n_ids, int(batch_bytes))

    def classifyPaths(self):
        """(sequences, or pairs, walked with their table in LDS, in HBM) of the last classify / classifyPairs call"""
        out = (C.c_uint64 * 2)()
        check(self._L.btlbf_mibf_classify_paths(self._h, out))
        return int(out[0]), int(out[1])

    def decode(self, values):
        """raw T values -> (id, saturated) as the reference's pair (v & antiMask, v > mask)"""
        v = np.asarray(values).astype(self.dtype)
        return v & self.dtype(self.mask - 1), v > self.dtype(self.mask)

    def data(self):
        out = np.zeros(max(self.getPop(), 1), self.dtype)
        check(self._L.btlbf_mibf_download(self._h, C.c_void_p(out.ctypes.data)))
        return out[: self.getPop()]

    def upload(self, data):
        a = np.ascontiguousarray(data, self.dtype)
        assert a.size == self.getPop()
        check(self._L.btlbf_mibf_upload(self._h, C.c_void_p(a.ctypes.data)))

    def counts(self):
        out = np.zeros(max(self.getPop(), 1), self.dtype)
        check(self._L.btlbf_mibf_download_counts(self._h, C.c_void_p(out.ctypes.data)))
        return out[: self.getPop()]

    def _stats(self):
        out = (C.c_uint64 * 3)()
        check(self._L.btlbf_mibf_stats(self._h, out))
        return list(out)

    def getPopNonZero(self):
        return self._stats()[1]

    def getPopSaturated(self):
        return self._stats()[2]

    def getIDCounts(self, n_ids):
        """getIDCounts (MIBloomFilter.hpp:539-551) -> (counts[n_ids], saturated total)"""
        counts = np.zeros(max(int(n_ids), 1), np.uint64)
        sat = C.c_uint64()
        check(self._L.btlbf_mibf_id_counts(self._h, C.c_void_p(counts.ctypes.data), int(n_ids), C.byref(sat)))
        return counts[: int(n_ids)], sat.value

    def store(self, path):
        check(self._L.btlbf_mibf_store(self._h, str(path).encode()))


class _ClassifyFile(_Owned):
    """the iterator behind MIBloomFilter.classifyFile: one batch per step, tally() for the running summary"""

    _destroy = "btlbf_mibf_classify_fastx_close"

    def __init__(self, mibf, p1, p2, flags, par, prob, minc, n_ids, batch_bytes):
        self._L = _lib.load()
        self._mibf = mibf  # the handle uses it until close()
        self.n_ids, self.max_results = n_ids, par.max_results
        h = C.c_void_p()
        check(self._L.btlbf_mibf_classify_fastx_open(C.byref(h), mibf._h, p1, p2, flags, C.byref(par),
                                                     C.c_void_p(prob.ctypes.data), C.c_void_p(minc.ctypes.data), n_ids,
                                                     batch_bytes))
        self._h = h

    def __iter__(self):
        return self

    def __next__(self):
        if not self._h:
            raise StopIteration
        first, n = C.c_uint64(), C.c_uint64()
        ptrs = [C.c_void_p() for _ in range(4)]
        check(self._L.btlbf_mibf_classify_fastx_next(self._h, C.byref(first), C.byref(n), *[C.byref(p) for p in ptrs]))
        n = n.value
        if n == 0:
            raise StopIteration
        copy = lambda p, shape, dt: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=shape).astype(dt, copy=True)
        words = copy(ptrs[0], (n, self.max_results, 4), np.uint32)
        return (first.value, hits_from_words(words)) + tuple(copy(p, (n,), np.uint32) for p in ptrs[1:])

    def tally(self):
        """(best, any, totals) over the rows delivered so far (btlbf_mibf_classify_fastx_tally)"""
        best, any_, totals = (np.zeros(max(self.n_ids, 1), np.uint64), np.zeros(max(self.n_ids, 1), np.uint64),
                              np.zeros(6, np.uint64))
        check(self._L.btlbf_mibf_classify_fastx_tally(self._h, C.c_void_p(best.ctypes.data), C.c_void_p(any_.ctypes.data),
                                                      C.c_void_p(totals.ctypes.data)))
        return best[: self.n_ids], any_[: self.n_ids], totals


# -- read screen (btlbf_screen_*): every read against several bit filters in one pass -----------------------------
def _filter_handles(filters):
    filters = list(filters)
    arr = (C.c_void_p * max(len(filters), 1))(*[f._h for f in filters])
    return filters, arr


def screenSeqs(filters, seq, starts=None, read_len=0, min_fraction=0.0, min_hits=1, stream=None):
    """The reads of a sequence buffer against every filter of `filters` (BloomFilter objects of one k, hash count and
    seeds, up to 16) in one pass (btlbf_screen_seqs) -> (hits[n, F], valid[n], pass_bits[n]), uint32: valid[s] = the
    clean windows of sequence s, hits[s, j] = those found in filters[j] -- what containsSeqs + count_per_seq give per
    filter --, bit j of pass_bits[s] = valid > 0 and hits >= min_hits and hits >= min_fraction * valid.  Buffers as
    containsSeqs takes them (host memory, or torch tensors on the GPU and then results as int32 tensors); neither
    starts nor read_len: the buffer is one sequence."""
    filters, arr = _filter_handles(filters)
    b = _Buf(seq)
    lay, keep = _layout(starts, read_len, b.mem)
    n = lay.n_seqs if starts is not None else (b.nbytes // int(read_len) if read_len else 1)
    nf = len(filters)
    hits, p_hits = _out(b, (n, nf), np.uint32)
    valid, p_valid = _out(b, n, np.uint32)
    pb, p_pb = _out(b, n, np.uint32)
    par = _lib.ScreenParams(float(min_fraction), int(min_hits), 0)
    check(_lib.load().btlbf_screen_seqs(arr, nf, b.ptr, b.nbytes, C.byref(lay) if lay else None, C.byref(par), p_hits,
                                         p_valid, p_pb, b.mem, _stream_ptr(stream, b.keep)))
    return hits, valid, pb


def screen_tally(hits, valid, pass_bits, passed=None, best=None, totals=None, device=0, stream=None):
    """btlbf_screen_tally: adds the summary of screened rows to (passed[F], best[F], totals[4]) and returns them:
    rows passing filter j; rows whose passing filter with the most hits is j (ties: the lowest j); {rows, rows passing
    none, rows passing two or more, rows without a clean window}.  Host results with uint64 numpy totals, or device
    results (screenSeqs' tensors) with int64 tensors; the totals are made, zeroed, where they are not given."""
    b = _Buf(hits, np.uint32)
    n_rows = len(valid)
    nf = int(hits.shape[1])
    outs = []
    for x, n in ((passed, nf), (best, nf), (totals, 4)):
        if x is None:
            x, _ = _out(b, n, np.uint64)
        outs.append(x)
    args = [_Buf(x, np.uint32) for x in (valid, pass_bits)] + [_Buf(x, np.uint64) if b.mem == HOST else _Buf(x) for x in outs]
    if any(a.mem != b.mem for a in args):
        raise ValueError("screen_tally: all arrays live in one memory space")
    for x, a in zip(outs, args[2:]):
        if b.mem == HOST and a.keep is not x:
            raise ValueError("screen_tally: the totals are contiguous uint64 arrays")
    check(_lib.load().btlbf_screen_tally(b.ptr, args[0].ptr, args[1].ptr, n_rows, nf, args[2].ptr, args[3].ptr, args[4].ptr,
                                          b.mem, (b.keep.device.index or 0) if b.mem == DEVICE else device,
                                          _stream_ptr(stream, b.keep)))
    return tuple(outs)


def screenFile(filters, path, min_fraction=0.0, min_hits=1, batch_bytes=0, per_line=False, summary_only=False):
    """screenSeqs over the records of one FASTA / FASTQ file (plain or gzip), in file order (btlbf_screen_fastx_*): an
    iterator of (first_row, hits[n, F], valid[n], pass_bits[n]) per batch of at most batch_bytes bases (0: 64 MiB),
    numpy arrays copied out of the library's buffers; its tally() gives the running summary, close() ends it early.
    With summary_only=True no per-read result leaves the GPU and the call returns (passed[F], best[F], totals[4],
    stats) as screen_tally defines them, stats being the call's statistics (n_windows = the sum of valid)."""
    filters, arr = _filter_handles(filters)
    par = _lib.ScreenParams(float(min_fraction), int(min_hits), 0)
    flags = _lib.FASTX_LINES if per_line else 0
    nf = len(filters)
    if summary_only:
        passed, best, totals = np.zeros(max(nf, 1), np.uint64), np.zeros(max(nf, 1), np.uint64), np.zeros(4, np.uint64)
        st = _lib.FastxStats()
        check(_lib.load().btlbf_screen_fastx(arr, nf, str(path).encode(), flags, C.byref(par), int(batch_bytes),
                                              C.c_void_p(passed.ctypes.data), C.c_void_p(best.ctypes.data),
                                              C.c_void_p(totals.ctypes.data), C.byref(st)))
        return passed[:nf], best[:nf], totals, st.as_dict()
    return _ScreenFile(filters, arr, str(path).encode(), flags, par, int(batch_bytes))


class _ScreenFile(_Owned):
    """the iterator behind screenFile: one batch per step, tally() for the running summary"""

    _destroy = "btlbf_screen_fastx_close"

    def __init__(self, filters, arr, path, flags, par, batch_bytes):
        self._L = _lib.load()
        self._filters = filters  # the handle uses them until close()
        self.n_filters = len(filters)
        h = C.c_void_p()
        check(self._L.btlbf_screen_fastx_open(C.byref(h), arr, self.n_filters, path, flags, C.byref(par), batch_bytes))
        self._h = h

    def __iter__(self):
        return self

    def __next__(self):
        if not self._h:
            raise StopIteration
        first, n = C.c_uint64(), C.c_uint64()
        ptrs = [C.c_void_p() for _ in range(3)]
        check(self._L.btlbf_screen_fastx_next(self._h, C.byref(first), C.byref(n), *[C.byref(p) for p in ptrs]))
        n = n.value
        if n == 0:
            raise StopIteration
        copy = lambda p, shape: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=shape).copy()
        return first.value, copy(ptrs[0], (n, self.n_filters)), copy(ptrs[1], (n,)), copy(ptrs[2], (n,))

    def tally(self):
        """(passed, best, totals) over the rows delivered so far (btlbf_screen_fastx_tally)"""
        nf = self.n_filters
        passed, best, totals = np.zeros(nf, np.uint64), np.zeros(nf, np.uint64), np.zeros(4, np.uint64)
        check(self._L.btlbf_screen_fastx_tally(self._h, C.c_void_p(passed.ctypes.data), C.c_void_p(best.ctypes.data),
                                               C.c_void_p(totals.ctypes.data)))
        return passed, best, totals


class CardinalityEstimate:
    """what KmerCardinality.estimate and solve_spectrum return: distinct (F0), singletons (f1), occupancy (the share of
    the table's counters that are not zero), spectrum (numpy: spectrum[i - 1] = f_i, the distinct k-mers seen i times,
    i = 1 .. n_hist - 2), overflow_buckets, and -- from a sketch -- windows, clean_windows, sampled"""

    def __init__(self, est, f):
        for name, _ in est._fields_:
            setattr(self, name, getattr(est, name))
        self.spectrum = np.array(f[1:], np.float64)

    def at_least(self, T):
        """the distinct k-mers seen at least T times: distinct - (f_1 + ... + f_{T-1}); what a filter that takes the
        output of CountingBloomFilter.toBloomFilter(T) has to hold"""
        T = int(T)
        if T < 1 or T - 1 > self.spectrum.size:
            raise ValueError("at_least(T): T must be 1..%d for this spectrum" % (self.spectrum.size + 1))
        return float(self.distinct - self.spectrum[: T - 1].sum())

    def __repr__(self):
        return "CardinalityEstimate(distinct=%.6g, singletons=%.6g, occupancy=%.4f)" % (self.distinct, self.singletons,
                                                                                        self.occupancy)


def solve_spectrum(t, sample_bits, table_bits):
    """the estimate from a histogram t of a sketch's counters (t[i] counters equal to i, the last entry those at or above
    it; KmerCardinality.histogram): btlbf_card_solve, host arithmetic that needs no GPU"""
    t = np.ascontiguousarray(t, np.uint64)
    est = _lib.CardEstimate()
    f = np.zeros(max(t.size - 1, 1), np.float64)
    check(_lib.load().btlbf_card_solve(C.c_void_p(t.ctypes.data), t.size, int(sample_bits), int(table_bits), C.byref(est),
                                       C.c_void_p(f.ctypes.data)))
    return CardinalityEstimate(est, f)


class KmerCardinality(_Owned):
    """A sampled, bucketed k-mer sketch in HBM (btlbf_card_*): estimates the distinct k-mers of reads and how many of
    them occur once, twice, ... -- the numbers the filters above are sized from -- in one pass of a fused kernel.
    A window is sampled when the top sample_bits bits of its mixed canonical ntHash value are zero; a sampled window
    counts in one of 2^table_bits saturating 32-bit counters."""

    _destroy = "btlbf_card_destroy"

    def __init__(self, k, sample_bits=_lib.CARD_SAMPLE_BITS, table_bits=_lib.CARD_TABLE_BITS, device=0):
        self._L = _lib.load()
        self.k, self.sample_bits, self.table_bits, self.device = int(k), int(sample_bits), int(table_bits), int(device)
        h = C.c_void_p()
        check(self._L.btlbf_card_create(C.byref(h), self.k, self.sample_bits, self.table_bits, self.device))
        self._h = h

    def clear(self):
        check(self._L.btlbf_card_clear(self._h))

    def addSeqs(self, seq, starts=None, read_len=0, stream=None):
        """add the windows of a buffer (layouts, memory spaces and streams as BloomFilter.insertSeqs); calls accumulate"""
        b = _Buf(seq)
        lay, keep = _layout(starts, read_len, b.mem)
        check(self._L.btlbf_card_add_seqs(self._h, b.ptr, b.nbytes, C.byref(lay) if lay else None, b.mem,
                                          _stream_ptr(stream, b.keep)))

    def addFile(self, path, per_line=False, batch_bytes=0):
        """add the windows of a FASTA / FASTQ file, plain or gzip -> the call's statistics (n_windows = clean windows,
        n_hits = sampled windows)"""
        st = _lib.FastxStats()
        check(self._L.btlbf_card_add_fastx(self._h, str(path).encode(), _lib.FASTX_LINES if per_line else 0,
                                           int(batch_bytes), C.byref(st)))
        return st.as_dict()

    def merge(self, other):
        """add another sketch of the same k, sample_bits, table_bits and device: the sketch of both inputs"""
        check(self._L.btlbf_card_merge(self._h, other._h))
        return self

    def _download(self):
        table, totals = np.zeros(1 << self.table_bits, np.uint32), np.zeros(3, np.uint64)
        check(self._L.btlbf_card_download(self._h, C.c_void_p(table.ctypes.data), C.c_void_p(totals.ctypes.data)))
        return table, totals

    def table(self):
        return self._download()[0]

    def totals(self):
        """(windows, clean windows, sampled windows)"""
        return tuple(int(x) for x in self._download()[1])

    def upload(self, table, totals):
        table = np.ascontiguousarray(table, np.uint32)
        totals = np.ascontiguousarray(totals, np.uint64)
        if table.size != 1 << self.table_bits or totals.size != 3:
            raise ValueError("upload: a table of 2^%d counters and 3 totals" % self.table_bits)
        check(self._L.btlbf_card_upload(self._h, C.c_void_p(table.ctypes.data), C.c_void_p(totals.ctypes.data)))

    def histogram(self, n_hist):
        """t[i] = counters equal to i (i < n_hist - 1), t[n_hist - 1] = counters at or above n_hist - 1"""
        t = np.zeros(max(int(n_hist), 1), np.uint64)
        check(self._L.btlbf_card_histogram(self._h, C.c_void_p(t.ctypes.data), int(n_hist)))
        return t

    def estimate(self, n_hist=64):
        est = _lib.CardEstimate()
        f = np.zeros(max(int(n_hist) - 1, 1), np.float64)
        check(self._L.btlbf_card_estimate_now(self._h, int(n_hist), C.byref(est), C.c_void_p(f.ctypes.data)))
        return CardinalityEstimate(est, f)
