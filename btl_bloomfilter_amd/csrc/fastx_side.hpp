// csrc/fastx_side.hpp -- one FASTA / FASTQ file read ahead of its consumer: the sequential parser (btlbf_fastx_open / _next)
// on a thread of its own, handing over its pinned batches in file order.  Shared by the file classifier
// (host_mibf_fastx.cpp) and the miBF builder (host_mibf_build.cpp), whose results depend on the order of the sequences.
#pragma once
#include "../../include/btlbf.h"
#include "host_internal.hpp"

#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>

namespace btlbf {

inline double now_s()
{
	using namespace std::chrono;
	return duration<double>(steady_clock::now().time_since_epoch()).count();
}

struct HostBatch {
	const char* bases = nullptr;
	const uint64_t* starts = nullptr;
	uint64_t nb = 0, ns = 0; // ns == 0: end of input
};

// one file: its sequential parser on a thread of its own, at most two batches ahead of the consumer (the parser's two
// buffers: one batch is handed back, by release(), before the parser may overwrite it)
struct Side {
	btlbf_fastx* r = nullptr;
	std::thread th;
	std::mutex mu;
	std::condition_variable cv;
	std::deque<HostBatch> q;
	int credits = 2;
	bool abort = false;
	int rc = BTLBF_OK;
	std::string err;
	double seconds_parse = 0;
	bool holding = false; // the consumer has a batch of this side

	void run()
	{
		for (;;) {
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return credits > 0 || abort; });
				if (abort)
					return;
				--credits;
			}
			HostBatch b;
			const double t0 = now_s();
			const int e = btlbf_fastx_next(r, &b.bases, &b.nb, &b.starts, &b.ns);
			{
				std::lock_guard<std::mutex> lk(mu);
				seconds_parse += now_s() - t0;
				if (e) {
					rc = e;
					err = btlbf_last_error();
					b = HostBatch();
				}
				q.push_back(b);
			}
			cv.notify_all();
			if (e || b.ns == 0)
				return;
		}
	}
	// the next batch (ns == 0 at the end of input, and from then on); the one taken before goes back to the parser
	int take(HostBatch* out)
	{
		std::unique_lock<std::mutex> lk(mu);
		if (holding) {
			holding = false;
			++credits;
			cv.notify_all();
		}
		cv.wait(lk, [&] { return !q.empty(); });
		*out = q.front();
		if (rc && out->ns == 0)
			return btlbf_set_error(rc, "%s", err.c_str());
		if (out->ns) {
			q.pop_front();
			holding = true;
		}
		return BTLBF_OK;
	}
	void stop()
	{
		{
			std::lock_guard<std::mutex> lk(mu);
			abort = true;
		}
		cv.notify_all();
		if (th.joinable())
			th.join();
		if (r)
			btlbf_fastx_close(r);
		r = nullptr;
	}
};


} // namespace btlbf
