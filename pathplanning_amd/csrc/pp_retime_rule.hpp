// The arithmetic of a retime call (include/pp_hip.h, "decided waits written into the timetables"), as k_retime_tickets (pp_retime.hpp) runs it and
// as a plain C++ program can run it: the dwell of a row, the validity of a hold, the prefix of a plan's holds, the hold a row belongs to and the
// rewritten time.  The stop predicate and the arrival time are the timetable call's and the step time is the speed profile's; nothing here restates
// them.  Nothing needs the device or a map and nothing allocates; double arithmetic only, every expression written in the order the header defines
// it (the library is built without contraction; tests/cpp/test_retime_rule.cpp is too), so host and device give the same bits.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pp_timetable_rule.hpp" // ppm::is_stop and ppm::arrive_time (and, through it, ppv::step_time)

#if defined(__HIPCC__)
#define PPR_INLINE __host__ __device__ __forceinline__
#else
#define PPR_INLINE inline
#endif

namespace ppr {

/// a call lists no more holds for one plan than this (their prefix sums are 8 bytes each of the kernel's LDS)
constexpr int kMaxHolds = 1 << 10;

/// pp_retime_result::status
constexpr int kApplied = 0, kNoProfile = -1, kNotAStop = -2, kNegativeDwell = -3;

/// a pp_hold array seen as int32 (the row of hold h is at [h * 4 + 1]) and as double (its seconds at [h * 2 + 1])
constexpr int kHoldInts = 4, kHoldDoubles = 2;

/// delta_r: how long row r >= 1 of a profile's (s, v, t) rows stands, its time less the arrival the timetable call derives from row r - 1
PPR_INLINE double dwell(const double* rows, int r, double aAcc, double aDec) { return rows[3 * (size_t)r + 2] - ppm::arrive_time(rows, r, aAcc, aDec); }

/// A hold of `seconds` at row r of a profile of N rows: kApplied if it is valid, else the status it gives its plan.  The stop test comes first.  (A
/// row outside 1 .. N - 1 never reaches the kernel: the host refuses it.  Here it is no stop.)
PPR_INLINE int hold_status(const double* rows, int N, int r, double seconds, double aAcc, double aDec)
{
	if (r < 1 || r >= N || !ppm::is_stop(rows[3 * (size_t)r + 1]))
		return kNotAStop;
	return dwell(rows, r, aAcc, aDec) + seconds >= 0.0 ? kApplied : kNegativeDwell;
}

/// P_0 = seconds_0, P_h = P_{h-1} + seconds_h, in list order; seconds_h = secondsOf[h * stride].  Returns the last P (0 for no hold).
PPR_INLINE double prefix(const double* secondsOf, int stride, int count, double* P)
{
	double sum = 0.0;
	for (int h = 0; h < count; h++) {
		sum = h == 0 ? secondsOf[0] : sum + secondsOf[(size_t)h * (size_t)stride];
		P[h] = sum;
	}
	return sum;
}

/// h(k): the last of `count` holds, ascending by row, whose row is <= k: its index, or -1.  The row of hold h is rowOf[h * stride].
PPR_INLINE int hold_of(const int32_t* rowOf, int stride, int count, int k)
{
	int lo = 0, hi = count; // the first h in 0 .. count with row_h > k (count: none)
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (rowOf[(size_t)mid * (size_t)stride] > k)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo - 1;
}

/// t'_k: one addition
PPR_INLINE double retimed(double t, double P) { return t + P; }

} // namespace ppr
