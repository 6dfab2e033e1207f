// The rule of prioritised start delays on the conflicts lattice (include/pp_hip.h, "start delays that clear conflicts"), as k_delay_level
// (pp_deconflict.hpp) and the host side of the call (pp_planner.hip) run it and as a plain C++ program can run it: which column of a vehicle's
// extended trajectory a lattice time reads under a delay, the key that orders the conflicts of a candidate and names its blocker, the list of
// a vehicle's lower-index partners (CSR), the level a vehicle is decided on, and the vehicles grouped by level.  Integer arithmetic only, no
// library function, no allocation: the caller brings every array.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pp_conflict_rule.hpp" // the pair list is the conflict call's: pairs == nullptr means every i < j, ppc::pair_of

#if defined(__HIPCC__)
#define PPY_INLINE __host__ __device__ __forceinline__
#else
#define PPY_INLINE inline
#endif

namespace ppy {

/// "no conflict" is "no key": above every key there is
constexpr uint64_t kNoKey = ~(uint64_t)0;

/// The extended trajectory has T + D columns, over lattice indices k0 - D .. k1 with the undelayed start.  At lattice time k0 + m (0 <= m < T) a
/// vehicle delayed by d steps (0 <= d <= D) is where that trajectory has column m + D - d: inside 0 .. T + D - 1 for every such m and d
PPY_INLINE int64_t column(int64_t m, int64_t D, int64_t d) { return m + D - d; }

/// the conflict of a candidate at lattice time m with partner j (an index into the call's n plans): ordered by (m, j), compared as integers
PPY_INLINE uint64_t key(int64_t m, int64_t n, int64_t j) { return (uint64_t)m * (uint64_t)n + (uint64_t)j; }
PPY_INLINE bool before(uint64_t key, uint64_t best) { return key < best; }
PPY_INLINE int32_t time_of(uint64_t key, int64_t n) { return (int32_t)(key / (uint64_t)n); }
PPY_INLINE int32_t partner_of(uint64_t key, int64_t n) { return (int32_t)(key % (uint64_t)n); }

/// pair p of a call's list: pairs[p], or -- pairs == nullptr -- the p-th pair i < j in row-major order
PPY_INLINE void pair_at(int n, const int32_t* pairs, int64_t p, int& a, int& b)
{
	if (pairs) {
		a = pairs[2 * p];
		b = pairs[2 * p + 1];
	} else
		ppc::pair_of(n, p, a, b);
}

/// offsets[0 .. n]: vehicle i's lower-index partners are list[offsets[i] .. offsets[i + 1]).  Of a pair (a, b) the larger index yields and lists
/// the smaller one; a pair given twice is listed twice (harmless: the same key).  Indices are 0 .. n - 1 and a != b (the call has checked).
PPY_INLINE void partner_offsets(int n, int64_t nPairs, const int32_t* pairs, int32_t* offsets)
{
	for (int i = 0; i <= n; i++)
		offsets[i] = 0;
	for (int64_t p = 0; p < nPairs; p++) {
		int a, b;
		pair_at(n, pairs, p, a, b);
		offsets[(a > b ? a : b) + 1]++;
	}
	for (int i = 0; i < n; i++)
		offsets[i + 1] += offsets[i];
}
/// ... and the list, in the order of the pair list; cursor[0 .. n - 1] is scratch
PPY_INLINE void partner_list(int n, int64_t nPairs, const int32_t* pairs, const int32_t* offsets, int32_t* cursor, int32_t* list)
{
	for (int i = 0; i < n; i++)
		cursor[i] = offsets[i];
	for (int64_t p = 0; p < nPairs; p++) {
		int a, b;
		pair_at(n, pairs, p, a, b);
		const int hi = a > b ? a : b, lo = a > b ? b : a;
		list[cursor[hi]++] = lo;
	}
}

/// level(i) = 0 without a partner j < i, else 1 + max level(j): a vehicle is decided one launch behind the last of its partners.  Returns the
/// number of levels (0 for n == 0).  Partners have smaller indices, so one ascending pass does it.
PPY_INLINE int levels(int n, const int32_t* offsets, const int32_t* list, int32_t* level)
{
	int count = 0;
	for (int i = 0; i < n; i++) {
		int32_t l = 0;
		for (int32_t k = offsets[i]; k < offsets[i + 1]; k++)
			if (level[list[k]] + 1 > l)
				l = level[list[k]] + 1;
		level[i] = l;
		if (l + 1 > count)
			count = l + 1;
	}
	return count;
}

/// the vehicles grouped by level, ascending index within a level: level l has members[first[l] .. first[l + 1]); first[0 .. nLevels]
PPY_INLINE void members_by_level(int n, int nLevels, const int32_t* level, int32_t* first, int32_t* members)
{
	for (int l = 0; l <= nLevels; l++)
		first[l] = 0;
	for (int i = 0; i < n; i++)
		first[level[i] + 1]++;
	for (int l = 0; l < nLevels; l++)
		first[l + 1] += first[l];
	for (int i = 0; i < n; i++) // (first[l] is the cursor of level l: afterwards it is the level's end)
		members[first[level[i]]++] = i;
	for (int l = nLevels; l > 0; l--)
		first[l] = first[l - 1];
	first[0] = 0;
}

} // namespace ppy
