// csrc/wide_counter.hpp -- device operations on counters wider than a byte (CountingBloomFilter<T>, T = uint16_t,
// uint32_t, uint64_t): the counterparts of cbf_read_fresh / cbf_inc_sat / cbf_cas_byte (device_utils.hpp), one template
// over the counter's width in bytes.  `base` is the filter's array, `p` a counter index.
//   2 bytes: the halfword (p & 1) of a 32-bit word; HBM has no halfword atomics, so the word is compared and swapped.
//            The addend is 1 << shift on a halfword that is below 0xffff, so it never carries into the neighbour;
//   4 and 8 bytes: the counter itself is compared and swapped.
#pragma once
#include "device_utils.hpp"

namespace btlbf {

template <int BYTES>
struct WideCtr;

template <>
struct WideCtr<2> {
	using V = uint32_t; // a counter's value in registers
	static constexpr V kMax = 0xffffu;
	// plain load for queries (random, never reused: non-temporal like bf_word)
	__device__ __forceinline__ static V load(const void* base, uint64_t p)
	{
		return __builtin_nontemporal_load(static_cast<const uint16_t*>(base) + p);
	}
	// agent-scope relaxed read: sees the other lanes' compare-and-swaps
	__device__ __forceinline__ static V read_fresh(const void* base, uint64_t p)
	{
		return (agent_load(static_cast<const uint32_t*>(base) + (p >> 1)) >> (((uint32_t)p & 1) * 16)) & kMax;
	}
	// saturating +1 (incrementAll's per-counter step, CountingBloomFilter.hpp:171-181)
	__device__ __forceinline__ static void inc_sat(void* base, uint64_t p)
	{
		uint32_t* w = static_cast<uint32_t*>(base) + (p >> 1);
		const uint32_t sh = ((uint32_t)p & 1) * 16;
		uint32_t old = agent_load(w);
		for (;;) {
			if (((old >> sh) & kMax) == kMax)
				return; // "newVal < currentVal": leave MAX alone
			const uint32_t prev = atomicCAS(w, old, old + (1u << sh));
			if (prev == old)
				return;
			old = prev;
		}
	}
	// expect -> expect + 1 (expect < MAX); true when this call made the change (CountingBloomFilter.hpp:152).  A
	// failure that only the neighbouring halfword caused is retried for as long as the own one still holds `expect`
	__device__ __forceinline__ static bool cas_inc(void* base, uint64_t p, V expect)
	{
		uint32_t* w = static_cast<uint32_t*>(base) + (p >> 1);
		const uint32_t sh = ((uint32_t)p & 1) * 16;
		uint32_t old = agent_load(w);
		for (;;) {
			if (((old >> sh) & kMax) != expect)
				return false;
			const uint32_t prev = atomicCAS(w, old, old + (1u << sh));
			if (prev == old)
				return true;
			old = prev;
		}
	}
};

template <>
struct WideCtr<4> {
	using V = uint32_t;
	static constexpr V kMax = 0xffffffffu;
	__device__ __forceinline__ static V load(const void* base, uint64_t p)
	{
		return __builtin_nontemporal_load(static_cast<const uint32_t*>(base) + p);
	}
	__device__ __forceinline__ static V read_fresh(const void* base, uint64_t p)
	{
		return agent_load(static_cast<const uint32_t*>(base) + p);
	}
	__device__ __forceinline__ static void inc_sat(void* base, uint64_t p)
	{
		uint32_t* c = static_cast<uint32_t*>(base) + p;
		uint32_t old = agent_load(c);
		while (old != kMax) {
			const uint32_t prev = atomicCAS(c, old, old + 1u);
			if (prev == old)
				return;
			old = prev;
		}
	}
	__device__ __forceinline__ static bool cas_inc(void* base, uint64_t p, V expect)
	{
		return atomicCAS(static_cast<uint32_t*>(base) + p, expect, expect + 1u) == expect;
	}
};

template <>
struct WideCtr<8> {
	using V = uint64_t;
	static constexpr V kMax = ~0ull;
	__device__ __forceinline__ static V load(const void* base, uint64_t p)
	{
		return __builtin_nontemporal_load(static_cast<const uint64_t*>(base) + p);
	}
	__device__ __forceinline__ static V read_fresh(const void* base, uint64_t p)
	{
		return __hip_atomic_load(static_cast<const uint64_t*>(base) + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__device__ __forceinline__ static void inc_sat(void* base, uint64_t p)
	{
		unsigned long long* c = static_cast<unsigned long long*>(base) + p;
		unsigned long long old = read_fresh(base, p);
		while (old != kMax) {
			const unsigned long long prev = atomicCAS(c, old, old + 1ull);
			if (prev == old)
				return;
			old = prev;
		}
	}
	__device__ __forceinline__ static bool cas_inc(void* base, uint64_t p, V expect)
	{
		return atomicCAS(static_cast<unsigned long long*>(base) + p, (unsigned long long)expect,
		                 (unsigned long long)expect + 1ull) == expect;
	}
};

// a counter's value as the caller's array holds it (min_out of the _wide calls, element = the counter's width)
template <int BYTES>
__device__ __forceinline__ void wide_store(void* out, uint64_t i, typename WideCtr<BYTES>::V v)
{
	if (BYTES == 2)
		static_cast<uint16_t*>(out)[i] = (uint16_t)v;
	else if (BYTES == 4)
		static_cast<uint32_t*>(out)[i] = (uint32_t)v;
	else
		static_cast<uint64_t*>(out)[i] = (uint64_t)v;
}

// incrementMin, CountingBloomFilter.hpp:135-162, over a k-mer's h counters.  each_pos(g) calls g(p) for the index p of
// every one of them, in hash order; it is walked once per pass (positions are recomputed, not stored)
template <int BYTES, class E>
__device__ __forceinline__ void wide_increment_min(void* base, E&& each_pos)
{
	using C = WideCtr<BYTES>;
	for (;;) {
		typename C::V mn = C::kMax;
		each_pos([&](uint64_t p) {
			const typename C::V v = C::read_fresh(base, p);
			mn = v < mn ? v : mn;
		});
		if (mn == C::kMax)
			return; // "minVal > newVal": saturated
		bool done = false;
		each_pos([&](uint64_t p) { done |= C::cas_inc(base, p, mn); });
		if (done)
			return;
	}
}

} // namespace btlbf
