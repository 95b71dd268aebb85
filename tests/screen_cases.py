"""Inputs and expectations shared by the read screen's GPU tests (test_gpu_screen.py, test_gpu_screen_file.py,
test_gpu_cpp_screen.py).  No test of its own.

The ragged buffer holds the lengths at which the fused kernel can go wrong -- 0, 1, k-1, k, k+1, around a wave's 64
bytes of bitmap, a read of 150, around a tile of 2048 window starts, a tile plus k-1, and 5000 (several tiles) -- in
shuffled order, four times over, plus sequences with runs of N, lowercase bases and nothing but N: about 60 sequences
whose total length is no multiple of 64.  Expected values come from the path the screen replaces, containsSeqs +
count_per_seq per filter (existing_path), and from the CPU oracle (oracle_counts)."""
import numpy as np

# three filters of every ragged case: a power of two, no power of two (a multiple of 8, as every bit filter's size must
# be), and more than 2^32 bits of no power of two (reduce_mod's small-magic form)
SIZES3 = (1 << 16, 100000, (1 << 32) + (1 << 20) + 64)
SEEDS2 = ["1110111011101110111011101110111", "1101101101101101011011011011011"]  # weight 24 and 21 of k = 31


def random_bases(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n).astype(np.uint8)


def ragged_lengths(k):
    return [0, 1, k - 1, k, k + 1, 63, 64, 65, 150, 2047, 2048, 2049, 2048 + k - 1, 5000]


class Ragged:
    def __init__(self, k, seed):
        rng = np.random.RandomState(seed)
        lens = ragged_lengths(k) * 4
        rng.shuffle(lens)
        seqs = [random_bases(rng, n) for n in lens]
        with_n = random_bases(rng, 400)
        with_n[100:109] = ord("N")      # a run of N inside a sequence
        with_n[250] = ord("N")
        lower = np.frombuffer(bytes(random_bases(rng, 300)).lower(), np.uint8).copy()
        lower[150:] = random_bases(rng, 150)  # half lowercase, half uppercase
        all_n = np.full(150, ord("N"), np.uint8)
        for pos, s in ((7, with_n), (23, lower), (41, all_n)):
            seqs.insert(pos, s)
        big = max(range(len(seqs)), key=lambda i: seqs[i].size)
        seqs[big][2040:2060] = ord("N")  # ... and a longer one inside a sequence of several tiles
        if sum(s.size for s in seqs) % 64 == 0:
            seqs.append(random_bases(rng, 7))
        self.k, self.seqs = k, seqs
        self.buf = np.concatenate(seqs)
        self.starts = np.concatenate([[0], np.cumsum([s.size for s in seqs])]).astype(np.uint64)
        self.n = len(seqs)
        assert self.buf.size % 64 != 0 and 55 <= self.n <= 65


def oracle_bodies(oracle, seqs, sizes, h, k):
    """filter j holds every sequence i with i % len(sizes) == j"""
    bodies = [np.zeros(b // 8, np.uint8) for b in sizes]
    for i, s in enumerate(seqs):
        j = i % len(sizes)
        oracle.bf_insert_seq(bodies[j], sizes[j], h, k, s.tobytes())
    return bodies


def make_filters(bf, bodies, sizes, h, k, seeds=None):
    out = []
    for body, bits in zip(bodies, sizes):
        f = bf.BloomFilter(bits, h, k)
        if seeds:
            f.setSpacedSeeds(seeds, 1)
        if body is not None:
            f.upload(body)
        out.append(f)
    return out


def oracle_counts(oracle, seqs, bodies, sizes, h, k):
    hits = np.zeros((len(seqs), len(sizes)), np.uint32)
    valid = np.zeros(len(seqs), np.uint32)
    for i, s in enumerate(seqs):
        for j, (body, bits) in enumerate(zip(bodies, sizes)):
            hit, ok = oracle.bf_contains_seq_dense(body, bits, h, k, s.tobytes())
            hits[i, j] = int((hit.astype(bool) & ok.astype(bool)).sum())
            valid[i] = int(ok.astype(bool).sum())
    return hits, valid


def existing_path(bf, filters, buf, k, starts=None, read_len=0):
    """the loop the screen replaces: containsSeqs + count_per_seq per filter, on host buffers -> (hits[n, F], valid[n])"""
    cols, valid = [], None
    for f in filters:
        hit, ok, _ = f.containsSeqs(buf, starts=starts, read_len=read_len)
        h, v = bf.count_per_seq(hit, ok, len(buf), k, starts=starts, read_len=read_len)
        cols.append(np.asarray(h).astype(np.uint32))
        assert valid is None or (valid == v).all()
        valid = np.asarray(v).astype(np.uint32)
    return np.stack(cols, axis=1), valid


def host(x):
    """a result array of screenSeqs as uint32 numpy (device results are int32 tensors)"""
    if not isinstance(x, np.ndarray):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint32) if x.dtype != np.uint32 else x


def fastq_bytes(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r.tobytes(), b"I" * r.size) for i, r in enumerate(reads))


def fasta_bytes(reads, wrap=70):
    out = []
    for i, r in enumerate(reads):
        s = r.tobytes()
        out.append(b">r%d\n" % i + b"".join(s[a:a + wrap] + b"\n" for a in range(0, len(s), wrap)))
    return b"".join(out)
