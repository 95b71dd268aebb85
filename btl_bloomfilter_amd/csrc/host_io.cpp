// csrc/host_io.cpp -- BTLBloomFilter_v1 / BTLCountingBloomFilter_v1 files: header text, header parsing, load, store.
//
// Files are read and written byte-for-byte the way the reference does (BloomFilter.hpp:107-166,264-314;
// CountingBloomFilter.hpp:268-368); the body streams through a pinned bounce buffer.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <sys/stat.h>
#include <unistd.h>

using namespace btlbf;

namespace {

// ---- header text ---------------------------------------------------------------------------
std::string toml_double(double v) // cpptoml.h:3477-3494
{
	char buf[64];
	snprintf(buf, sizeof buf, "%#.17g", v);
	std::string s(buf);
	size_t p = s.find("e0");
	if (p != std::string::npos)
		s.replace(p, 2, "e");
	p = s.find("e-0");
	if (p != std::string::npos)
		s.replace(p, 3, "e-");
	return s;
}

// Key order: what libstdc++'s unordered_map yields for the reference's insertion order
// (cpptoml.h:43-52,3332; BloomFilter.hpp:275-281; CountingBloomFilter.hpp:355-359)
std::string header_text(const btlbf_filter* f)
{
	char buf[640];
	if (f->kind == BTLBF_BLOOM) {
		snprintf(buf, sizeof buf,
		         "[BTLBloomFilter_v1]\n\tnEntry = %llu\n\tdFPR = %s\n\tEntry = %llu\n"
		         "\tBloomFilterSizeInBytes = %llu\n\tBloomFilterSize = %llu\n\tHashNum = %u\n"
		         "\tKmerSize = %u\n[HeaderEnd]\n",
		         (unsigned long long)f->n_entry, toml_double(f->dfpr).c_str(),
		         (unsigned long long)f->t_entry, (unsigned long long)f->size_bytes,
		         (unsigned long long)f->size, f->h, f->k);
	} else {
		snprintf(buf, sizeof buf,
		         "[BTLCountingBloomFilter_v1]\n\tBloomFilterSize = %llu\n\tHashNum = %u\n"
		         "\tKmerSize = %u\n\tBloomFilterSizeInBytes = %llu\n\tBitsPerCounter = %u\n"
		         "[HeaderEnd]\n",
		         (unsigned long long)f->size, f->h, f->k, (unsigned long long)f->size_bytes,
		         f->bits_per_counter);
	}
	return buf;
}

std::string trim(const std::string& s)
{
	size_t a = s.find_first_not_of(" \t\r");
	if (a == std::string::npos)
		return "";
	size_t b = s.find_last_not_of(" \t\r");
	return s.substr(a, b - a + 1);
}

struct ParsedHeader {
	bool has[8] = {false};
	uint64_t size = 0, size_bytes = 0, n_entry = 0, t_entry = 0;
	unsigned h = 0, k = 0, bits_per_counter = 8;
	double dfpr = 0;
	size_t header_len = 0;
};

// Order-insensitive reader of the "key = value" lines between the magic line and [HeaderEnd]
// (the reference hands them to a TOML parser, BloomFilter.hpp:118-166).
int parse_header(FILE* fp, int kind, const char* path, ParsedHeader& out)
{
	const char* magic = kind == BTLBF_BLOOM ? "[BTLBloomFilter_v1]" : "[BTLCountingBloomFilter_v1]";
	std::string line;
	auto getline = [&](std::string& l) -> bool {
		l.clear();
		int c;
		bool any = false;
		while ((c = fgetc(fp)) != EOF) {
			any = true;
			out.header_len++;
			if (c == '\n')
				return true;
			l.push_back((char)c);
			if (l.size() > 4096)
				return true;
		}
		return any;
	};
	if (!getline(line) || line != magic)
		return fail(BTLBF_EFORMAT,
		            "%s: magic string does not match (likely version mismatch): got \"%.60s\", want \"%s\"",
		            path, line.c_str(), magic);
	bool end = false;
	while (getline(line)) {
		if (line == "[HeaderEnd]") {
			end = true;
			break;
		}
		const size_t eq = line.find('=');
		if (eq == std::string::npos)
			continue;
		const std::string key = trim(line.substr(0, eq)), val = trim(line.substr(eq + 1));
		if (key == "BloomFilterSize") {
			out.size = strtoull(val.c_str(), nullptr, 10);
			out.has[0] = true;
		} else if (key == "HashNum") {
			out.h = (unsigned)strtoul(val.c_str(), nullptr, 10);
			out.has[1] = true;
		} else if (key == "KmerSize") {
			out.k = (unsigned)strtoul(val.c_str(), nullptr, 10);
			out.has[2] = true;
		} else if (key == "BloomFilterSizeInBytes") {
			out.size_bytes = strtoull(val.c_str(), nullptr, 10);
			out.has[3] = true;
		} else if (key == "dFPR") {
			out.dfpr = strtod(val.c_str(), nullptr);
			out.has[4] = true;
		} else if (key == "nEntry") {
			out.n_entry = strtoull(val.c_str(), nullptr, 10);
			out.has[5] = true;
		} else if (key == "Entry") {
			out.t_entry = strtoull(val.c_str(), nullptr, 10);
			out.has[6] = true;
		} else if (key == "BitsPerCounter") {
			out.bits_per_counter = (unsigned)strtoul(val.c_str(), nullptr, 10);
			out.has[7] = true;
		}
	}
	if (!end)
		return fail(BTLBF_EFORMAT, "%s: pre-built bloom filter does not have the correct header end", path);
	const int need_bloom[] = {0, 1, 2, 3, 4, 5, 6}, need_cnt[] = {0, 1, 2, 3, 7};
	if (kind == BTLBF_BLOOM) {
		for (int i : need_bloom)
			if (!out.has[i])
				return fail(BTLBF_EFORMAT, "%s: header key missing", path);
	} else {
		for (int i : need_cnt)
			if (!out.has[i])
				return fail(BTLBF_EFORMAT, "%s: header key missing", path);
	}
	return BTLBF_OK;
}

// Does the header of a counting file fit the kind it is loaded as?  BTLBF_COUNTING8 keeps its own rule; a wide kind of w
// bytes per counter needs BloomFilterSize * w == BloomFilterSizeInBytes -- BitsPerCounter is not trusted for the width (the
// reference writes 8 for every T, CountingBloomFilter.hpp:109,357).  The reference itself does not check and would
// silently misread.  No HIP call on the way to the error (the file is the caller's to close).
int check_counting_header(int kind, const ParsedHeader& ph, const char* path)
{
	const uint64_t w = (uint64_t)kind_counter_bytes(kind);
	if (w == 1) {
		if (ph.bits_per_counter != 8 || ph.size != ph.size_bytes)
			return fail(BTLBF_EFORMAT, "%s: only 8-bit counters are supported (BitsPerCounter = %u)", path,
			            ph.bits_per_counter);
		return BTLBF_OK;
	}
	if (ph.size == 0 || ph.size > ~0ull / w || ph.size * w != ph.size_bytes)
		return btlbf_set_error(BTLBF_EFORMAT,
		                       "%s: BloomFilterSize = %llu counters of %llu bytes do not make BloomFilterSizeInBytes = %llu: "
		                       "not a filter of %llu-bit counters",
		                       path, (unsigned long long)ph.size, (unsigned long long)w,
		                       (unsigned long long)ph.size_bytes, (unsigned long long)(8 * w));
	return BTLBF_OK;
}

} // namespace

// -------------------------------------------------------------------------------------------------
// files
// -------------------------------------------------------------------------------------------------
extern "C" int btlbf_header(const btlbf_filter* f, char* buf, size_t cap, size_t* len)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	const std::string h = header_text(f);
	if (len)
		*len = h.size();
	if (buf) {
		if (cap < h.size())
			return fail(BTLBF_EINVAL, "header buffer too small (%zu < %zu)", cap, h.size());
		memcpy(buf, h.data(), h.size());
	}
	return BTLBF_OK;
}

extern "C" int btlbf_load(btlbf_filter** out, int kind, const char* path, unsigned threshold, int device)
{
	if (!out || !path)
		return fail(BTLBF_EINVAL, "null argument");
	*out = nullptr;
	if (kind_counter_bytes(kind) < 0)
		return btlbf_set_error(BTLBF_EINVAL, "unknown filter kind %d", kind);
	FILE* fp = fopen(path, "rb");
	if (!fp)
		return fail(BTLBF_EIO, "error: `%s': %s", path, strerror(errno));
	ParsedHeader ph;
	int rc = parse_header(fp, kind, path, ph);
	if (rc) {
		fclose(fp);
		return rc;
	}
	btlbf_filter* f = nullptr;
	if (kind == BTLBF_BLOOM) {
		if (ph.size % 8 != 0) {
			fclose(fp);
			return fail(BTLBF_EINVAL, "ERROR: Filter Size \"%llu\" is not a multiple of 8.",
			            (unsigned long long)ph.size);
		}
		rc = make_filter(&f, kind, ph.size, ph.size / 8, 0, 1, ph.h, ph.k, 0, device);
	} else {
		if ((rc = check_counting_header(kind, ph, path))) {
			fclose(fp);
			return rc;
		}
		rc = make_filter(&f, kind, ph.size, ph.size_bytes, 0, 1, ph.h, ph.k, threshold, device);
	}
	if (rc) {
		fclose(fp);
		return rc;
	}
	f->bits_per_counter = ph.bits_per_counter; // echoed by store (8 for every 8-bit file, checked above)
	f->dfpr = ph.dfpr;
	f->n_entry = ph.n_entry;
	f->t_entry = ph.t_entry;
	{
		DeviceGuard g0(device);
		if (materialize_clear(f, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
			fclose(fp);
			btlbf_destroy(f);
			return fail(BTLBF_EHIP, "clearing the filter failed");
		}
	}
	// body: stream through a pinned bounce buffer
	const size_t chunk = 64u << 20;
	void* bounce = nullptr;
	DeviceGuard g(device);
	if (hipHostMalloc(&bounce, chunk, hipHostMallocDefault) != hipSuccess) {
		fclose(fp);
		btlbf_destroy(f);
		return fail(BTLBF_ENOMEM, "pinned bounce buffer");
	}
	uint64_t done = 0;
	while (done < f->local_bytes) {
		const size_t n = (size_t)std::min<uint64_t>(chunk, f->local_bytes - done);
		if (fread(bounce, 1, n, fp) != n) {
			(void)hipHostFree(bounce);
			fclose(fp);
			btlbf_destroy(f);
			return fail(BTLBF_EIO, "error: `%s': short read of the filter body", path);
		}
		if (hipMemcpy(static_cast<uint8_t*>(f->d_data) + done, bounce, n, hipMemcpyHostToDevice) != hipSuccess) {
			(void)hipHostFree(bounce);
			fclose(fp);
			btlbf_destroy(f);
			return fail(BTLBF_EHIP, "upload of the filter body failed");
		}
		done += n;
	}
	(void)hipHostFree(bounce);
	fclose(fp);
	*out = f;
	return BTLBF_OK;
}

// A zeroed filter with the geometry and the bookkeeping fields of a header text (everything up to and including
// the "[HeaderEnd]" line): what the reference's public loadHeader(std::istream&) leaves behind
// (BloomFilter.hpp:118-166, CountingBloomFilter.hpp:84,282-343) before loadFilter reads the body.
extern "C" int btlbf_create_from_header(btlbf_filter** out, int kind, const char* header, size_t len, unsigned threshold,
                                        int device)
{
	if (!out || !header)
		return fail(BTLBF_EINVAL, "null argument");
	*out = nullptr;
	if (kind_counter_bytes(kind) < 0)
		return btlbf_set_error(BTLBF_EINVAL, "unknown filter kind %d", kind);
	FILE* fp = fmemopen(const_cast<char*>(header), len, "rb");
	if (!fp)
		return fail(BTLBF_EIO, "fmemopen: %s", strerror(errno));
	ParsedHeader ph;
	int rc = parse_header(fp, kind, "<header>", ph);
	fclose(fp);
	if (rc)
		return rc;
	btlbf_filter* f = nullptr;
	if (kind == BTLBF_BLOOM) {
		if (ph.size % 8 != 0)
			return fail(BTLBF_EINVAL, "ERROR: Filter Size \"%llu\" is not a multiple of 8.", (unsigned long long)ph.size);
		rc = make_filter(&f, kind, ph.size, ph.size / 8, 0, 1, ph.h, ph.k, 0, device);
	} else {
		if (kind == BTLBF_COUNTING8 && (ph.bits_per_counter != 8 || ph.size != ph.size_bytes))
			return fail(BTLBF_EFORMAT, "only 8-bit counters are supported (BitsPerCounter = %u)", ph.bits_per_counter);
		if (kind != BTLBF_COUNTING8 && (rc = check_counting_header(kind, ph, "<header>")))
			return rc;
		rc = make_filter(&f, kind, ph.size, ph.size_bytes, 0, 1, ph.h, ph.k, threshold, device);
	}
	if (rc)
		return rc;
	f->bits_per_counter = ph.bits_per_counter;
	f->dfpr = ph.dfpr;
	f->n_entry = ph.n_entry;
	f->t_entry = ph.t_entry;
	*out = f;
	return BTLBF_OK;
}

extern "C" double btlbf_get_dfpr(const btlbf_filter* f) { return f ? f->dfpr : 0.0; }
extern "C" void btlbf_set_dfpr(btlbf_filter* f, double v)
{
	if (f)
		f->dfpr = v;
}

static int write_body(const btlbf_filter* f, int fd, uint64_t file_off, const char* path)
{
	const size_t chunk = 64u << 20;
	void* bounce = nullptr;
	if (hipHostMalloc(&bounce, chunk, hipHostMallocDefault) != hipSuccess)
		return fail(BTLBF_ENOMEM, "pinned bounce buffer");
	uint64_t done = 0;
	int rc = BTLBF_OK;
	while (done < f->local_bytes && rc == BTLBF_OK) {
		const size_t n = (size_t)std::min<uint64_t>(chunk, f->local_bytes - done);
		if (hipMemcpy(bounce, static_cast<const uint8_t*>(f->d_data) + done, n, hipMemcpyDeviceToHost) !=
		    hipSuccess) {
			rc = fail(BTLBF_EHIP, "download of the filter body failed");
			break;
		}
		size_t w = 0;
		while (w < n) {
			ssize_t r = pwrite(fd, static_cast<const char*>(bounce) + w, n - w, (off_t)(file_off + done + w));
			if (r <= 0) {
				rc = fail(BTLBF_EIO, "error: `%s': %s", path, strerror(errno));
				break;
			}
			w += (size_t)r;
		}
		done += n;
	}
	(void)hipHostFree(bounce);
	return rc;
}

static int store_locked(btlbf_filter* f, const char* path);

extern "C" int btlbf_store_shard(btlbf_filter* f, const char* path)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_store_shard");
	return store_locked(f, path);
}

// header + body of the local array at its place in the file; the caller holds the filter's lock
static int store_locked(btlbf_filter* f, const char* path)
{
	if (!f || !path)
		return fail(BTLBF_EINVAL, "null argument");
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize());
	const std::string hdr = header_text(f);
	const int flags = O_WRONLY | O_CREAT | (f->shard_count == 1 ? O_TRUNC : 0);
	const int fd = open(path, flags, 0644);
	if (fd < 0)
		return fail(BTLBF_EIO, "error: `%s': %s", path, strerror(errno));
	int rc = BTLBF_OK;
	if (f->shard_index == 0) {
		if (pwrite(fd, hdr.data(), hdr.size(), 0) != (ssize_t)hdr.size())
			rc = fail(BTLBF_EIO, "error: `%s': %s", path, strerror(errno));
		if (rc == BTLBF_OK && f->shard_count > 1 && ftruncate(fd, (off_t)(hdr.size() + f->size_bytes)) != 0)
			rc = fail(BTLBF_EIO, "error: `%s': %s", path, strerror(errno));
	}
	if (rc == BTLBF_OK)
		rc = write_body(f, fd, hdr.size() + (uint64_t)f->shard_index * f->local_bytes, path);
	if (close(fd) != 0 && rc == BTLBF_OK)
		rc = fail(BTLBF_EIO, "error: `%s': %s", path, strerror(errno));
	return rc;
}

extern "C" int btlbf_store(btlbf_filter* f, const char* path)
{
	FilterLock lk__(f);
	if (f && f->shard_count != 1)
		return fail(BTLBF_EINVAL, "btlbf_store on a shard: use btlbf_store_shard");
	return store_locked(f, path);
}
