// tests/cpp/stub_abi_card.cpp -- TEST-ONLY: the entry points btlbf::KmerCardinality (include/btlbf/KmerCardinality.hpp)
// calls, without the library and without a GPU, for tests/cpp/test_card_shim.cpp.  A "sketch" here is a host table that
// add_seqs bumps once per SEQUENCE at the sequence's length (mod the table), so that the program can tell what the class
// passed down -- buffers, offsets, flags, sizes -- and that what comes back reaches the caller in the right fields.  The
// solver hands back recognisable numbers, not estimates.  The log of calls is stub_card_log().
#include "../../include/btlbf.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct btlbf_card {
	unsigned k, s, r;
	int device;
	std::vector<uint32_t> table;
	uint64_t tot[3];
};

static std::string g_log, g_err;
static int g_live = 0;
const std::string& stub_card_log() { return g_log; }
int stub_card_live() { return g_live; }
static void logf(const char* fmt, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0,
                 unsigned long long d = 0)
{
	char buf[256];
	std::snprintf(buf, sizeof buf, fmt, a, b, c, d);
	g_log += buf;
	g_log += '\n';
}
static int err(int code, const char* msg)
{
	g_err = msg;
	return code;
}

extern "C" {
const char* btlbf_last_error(void) { return g_err.c_str(); }

int btlbf_card_create(btlbf_card** out, unsigned k, unsigned s, unsigned r, int device)
{
	*out = nullptr;
	if (r < 6 || r > 28)
		return err(BTLBF_EINVAL, "stub: table_bits");
	btlbf_card* c = new btlbf_card{k, s, r, device, std::vector<uint32_t>(size_t(1) << r, 0), {0, 0, 0}};
	++g_live;
	logf("create %llu %llu %llu %llu", k, s, r, (unsigned long long)device);
	*out = c;
	return BTLBF_OK;
}
void btlbf_card_destroy(btlbf_card* c)
{
	if (c)
		--g_live;
	delete c;
}
int btlbf_card_clear(btlbf_card* c)
{
	c->table.assign(c->table.size(), 0);
	c->tot[0] = c->tot[1] = c->tot[2] = 0;
	logf("clear");
	return BTLBF_OK;
}
int btlbf_card_add_seqs(btlbf_card* c, const char* seq, uint64_t len, const btlbf_layout* l, int mem, void* stream)
{
	if (len && !seq)
		return err(BTLBF_EINVAL, "stub: null sequence");
	const uint64_t n = l && l->starts ? l->n_seqs : 1;
	logf("add_seqs len %llu seqs %llu mem %llu stream %llu", len, n, (unsigned long long)mem, stream ? 1 : 0);
	for (uint64_t i = 0; i < n; ++i) {
		const uint64_t b = l && l->starts ? l->starts[i] : 0, e = l && l->starts ? l->starts[i + 1] : len;
		if (e < b || e > len)
			return err(BTLBF_EINVAL, "stub: offsets");
		c->table[(e - b) % c->table.size()] += 1;
		c->tot[0] += e - b >= c->k ? e - b - c->k + 1 : 0;
	}
	c->tot[1] = c->tot[0];
	c->tot[2] += n;
	return BTLBF_OK;
}
int btlbf_card_add_fastx(btlbf_card* c, const char* path, uint32_t flags, uint64_t batch_bytes, btlbf_fastx_stats* st)
{
	if (std::strstr(path, "missing"))
		return err(BTLBF_EIO, "stub: file could not be read");
	g_log += std::string("add_fastx ") + path + "\n";
	logf("add_fastx flags %llu batch %llu", flags, batch_bytes);
	if (st) {
		std::memset(st, 0, sizeof *st);
		st->n_records = 7;
		st->n_bases = 700;
		st->n_windows = 70;
	}
	c->table[7] += 1;
	return BTLBF_OK;
}
int btlbf_card_merge(btlbf_card* d, const btlbf_card* s)
{
	if (d->k != s->k || d->s != s->s || d->r != s->r)
		return err(BTLBF_EINVAL, "stub: merge of different sketches");
	for (size_t i = 0; i < d->table.size(); ++i)
		d->table[i] += s->table[i];
	for (int i = 0; i < 3; ++i)
		d->tot[i] += s->tot[i];
	return BTLBF_OK;
}
int btlbf_card_download(btlbf_card* c, uint32_t* table, uint64_t* tot)
{
	std::memcpy(table, c->table.data(), c->table.size() * 4);
	std::memcpy(tot, c->tot, sizeof c->tot);
	return BTLBF_OK;
}
int btlbf_card_upload(btlbf_card* c, const uint32_t* table, const uint64_t* tot)
{
	std::memcpy(c->table.data(), table, c->table.size() * 4);
	std::memcpy(c->tot, tot, sizeof c->tot);
	return BTLBF_OK;
}
int btlbf_card_histogram(btlbf_card* c, uint64_t* t, unsigned n_hist)
{
	if (n_hist < 3 || n_hist > 8192)
		return err(BTLBF_EINVAL, "stub: n_hist");
	std::memset(t, 0, n_hist * sizeof *t);
	for (uint32_t v : c->table)
		t[v < n_hist - 1 ? v : n_hist - 1] += 1;
	return BTLBF_OK;
}
int btlbf_card_solve(const uint64_t* t, unsigned n_hist, unsigned s, unsigned r, btlbf_card_estimate* e, double* f)
{
	if (!t || n_hist < 3 || n_hist > 8192)
		return err(BTLBF_EINVAL, "stub: n_hist");
	logf("solve %llu %llu %llu", n_hist, s, r);
	std::memset(e, 0, sizeof *e);
	for (unsigned i = 0; i + 1 < n_hist; ++i)
		f[i] = i ? 100.0 / i : 0.0;
	e->distinct = 1000.0 + (double)t[1];
	e->singletons = f[1];
	e->occupancy = 0.25;
	e->overflow_buckets = t[n_hist - 1];
	return BTLBF_OK;
}
int btlbf_card_estimate_now(btlbf_card* c, unsigned n_hist, btlbf_card_estimate* e, double* f)
{
	std::vector<uint64_t> t(n_hist < 3 ? 3 : n_hist);
	int rc = btlbf_card_histogram(c, t.data(), n_hist);
	if (rc || (rc = btlbf_card_solve(t.data(), n_hist, c->s, c->r, e, f)))
		return rc;
	e->windows = c->tot[0];
	e->clean_windows = c->tot[1];
	e->sampled = c->tot[2];
	return BTLBF_OK;
}
}
