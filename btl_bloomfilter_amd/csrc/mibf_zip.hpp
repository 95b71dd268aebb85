// csrc/mibf_zip.hpp -- pairing the records of two files whose parsers cut their batches by bytes (host only, no HIP:
// tests/cpp/test_mibf_zip.cpp checks it by brute force).  Side 0 delivers mate 1 of every pair, side 1 mate 2; a batch
// holds any number of records, zero included, and the two sides' batches end at unrelated records.  The zipper says
// what to do next:
//   NEED_0 / NEED_1 : feed(side, n_records, last) the next batch of that side (last: the side's input ends with it);
//   TAKE            : take() records of both current batches form pairs now -- from record pos(side) of each, which
//                     take() then moves on; the rest of the longer batch waits for the other side's next batch;
//   END             : both sides ended with every record paired;
//   UNEQUAL         : one side ended and the other still has a record: the files do not pair up.  Reported only once
//                     every pair that exists has been taken.
// No record is dropped or reordered: pair i is record i of side 0 and record i of side 1.
#pragma once
#include <cstdint>
#include <vector>

namespace btlbf {

// The offsets of the buffer in which n pairs are interleaved (mate 1 of pair 0, mate 2 of pair 0, mate 1 of pair 1, ...),
// from the offsets of the two sides' buffers, s1[0..n] and s2[0..n]: what interleave_mates_kernel writes on the device,
// in closed form.  A side's offsets need not start at 0 (a window of a batch); the result starts at s1[0] + s2[0].
inline std::vector<uint64_t> mibf_zip_starts(const uint64_t* s1, const uint64_t* s2, uint64_t n)
{
	std::vector<uint64_t> out(2 * n + 1);
	for (uint64_t i = 0; i < n; ++i) {
		out[2 * i] = s1[i] + s2[i];
		out[2 * i + 1] = s1[i + 1] + s2[i];
	}
	out[2 * n] = s1[n] + s2[n];
	return out;
}

struct MibfZip {
	enum Step { NEED_0 = 0, NEED_1 = 1, TAKE, END, UNEQUAL };
	uint64_t left[2] = {0, 0};  // records of the current batch not yet paired
	uint64_t at[2] = {0, 0};    // the first of them
	bool ended[2] = {false, false};
	uint64_t pairs = 0;         // pairs taken so far

	Step step() const
	{
		if (left[0] && left[1])
			return TAKE;
		// a side whose batch is used up is asked first: the other side's rest cannot pair without it
		for (int s = 0; s < 2; ++s)
			if (!left[s] && !ended[s])
				return s ? NEED_1 : NEED_0;
		return left[0] || left[1] ? UNEQUAL : END;
	}
	// the next batch of a side whose current one is used up
	void feed(int side, uint64_t n_records, bool last)
	{
		left[side] = n_records;
		at[side] = 0;
		ended[side] = last;
	}
	uint64_t pos(int side) const { return at[side]; }
	// pairs formed now: records [pos(0), pos(0) + n) of side 0 with [pos(1), pos(1) + n) of side 1
	uint64_t take()
	{
		const uint64_t n = left[0] < left[1] ? left[0] : left[1];
		for (int s = 0; s < 2; ++s) {
			left[s] -= n;
			at[s] += n;
		}
		pairs += n;
		return n;
	}
};

} // namespace btlbf
