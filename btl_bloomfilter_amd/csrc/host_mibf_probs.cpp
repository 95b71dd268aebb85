// csrc/host_mibf_probs.cpp -- btlbf_mibf_frame_probs: MIBloomFilter<T>::calcFrameProbs (MIBloomFilter.hpp:664-679), the
// table every caller of the classifier fills perFrameProb with.  The counts come from the device histogram of
// btlbf_mibf_id_counts; the arithmetic is the reference's, on the host, in double, in its order of operations.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"

#include <cmath>
#include <vector>

// the reference's results, bit for bit: no fused multiply-add may replace prob * x + probTotal (btlbf.h: the compareStdErr
// rule of btlbf_mibf_classify_seqs)
#pragma clang fp contract(off)
#pragma STDC FP_CONTRACT OFF

using namespace btlbf;

namespace {

// nChoosek (MIBloomFilter.hpp:781-796): the running product lives in an int, multiplied and divided in unsigned
unsigned n_choose_k(unsigned n, unsigned k)
{
	if (k > n)
		return 0;
	if (k * 2 > n)
		k = n - k;
	if (k == 0)
		return 1;
	int result = (int)n;
	for (unsigned i = 2; i <= k; ++i) {
		result = (int)((unsigned)result * (n - i + 1));
		result = (int)((unsigned)result / i);
	}
	return (unsigned)result;
}

} // namespace

// calcProbSingleFrame (MIBloomFilter.hpp:65-77).  allowed_misses > hash_num: the unsigned loop start wraps and the loop
// does not run, there as here: 0
extern "C" double btlbf_mibf_prob_single_frame(double occupancy, unsigned hash_num, double freq, unsigned allowed_misses)
{
	double prob_total = 0.0;
	for (unsigned i = hash_num - allowed_misses; i <= hash_num; i++) {
		double prob = n_choose_k(hash_num, i);
		prob *= std::pow(occupancy, (double)i);
		prob *= std::pow(1.0 - occupancy, (double)(hash_num - i));
		prob *= (1.0 - std::pow(1.0 - freq, (double)i));
		prob_total += prob;
	}
	return prob_total;
}

extern "C" int btlbf_mibf_frame_probs(btlbf_mibf* m, unsigned allowed_miss, double* frame_probs, uint64_t n,
                                      double* sat_prop)
{
	if (!m || !frame_probs || !sat_prop)
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	if (n == 0)
		return btlbf_set_error(BTLBF_EINVAL, "miBF frame probabilities: n must be at least 1");
	const unsigned h = btlbf_mibf_hash_num(m);
	if (allowed_miss > h)
		return btlbf_set_error(BTLBF_EINVAL, "miBF frame probabilities: allowed_miss %u is above the %u hash values of a frame; nothing "
		            "was written", allowed_miss, h);
	uint64_t max_id = 0;
	int rc = mibf_max_id(m, &max_id);
	if (rc)
		return rc;
	if (max_id >= n)
		return fail(BTLBF_EINVAL, "miBF frame probabilities: the ID array holds id %llu, the table %llu entries; nothing was "
		            "written", (unsigned long long)max_id, (unsigned long long)n);
	std::vector<uint64_t> count_table(n, 0);
	uint64_t saturated = 0;
	if ((rc = btlbf_mibf_id_counts(m, count_table.data(), n, &saturated)))
		return rc;
	uint64_t sum = 0;
	for (uint64_t i = 1; i < n; ++i)
		sum += count_table[i];
	if (sum == 0)
		return fail(BTLBF_EINVAL, "miBF frame probabilities: no entry of the ID array holds an id of 1..%llu; nothing was "
		            "written", (unsigned long long)(n - 1));
	const double occupancy = double(btlbf_mibf_size(m)) / double(btlbf_mibf_bits(m));
	*sat_prop = double(saturated) / double(sum);
	for (uint64_t i = 1; i < n; ++i)
		frame_probs[i] =
		    btlbf_mibf_prob_single_frame(occupancy, h, double(count_table[i]) / double(sum), allowed_miss);
	return BTLBF_OK;
}
