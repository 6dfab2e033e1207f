// The arithmetic of timetable look-ups and stops (include/pp_hip.h, "timetable look-ups and stops"), as k_timetable_tickets (pp_timetable.hpp)
// runs it and as a plain C++ program can run it: the row search by arc length, the time within a step of the profile from the position within it
// (the inverse of ppc::step_position), speed and acceleration at a time, the stop predicate, the arrival time of a stop and the search for the next
// stop.  Nothing here needs the device or a map and nothing allocates; double arithmetic only, every expression written in the order the header
// defines it (the library is built without contraction; tests/cpp/test_timetable_rule.cpp is too), so host and device give the same bits.  The
// only library function is the square root, the compiler's builtin: correctly rounded on either side.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pp_conflict_rule.hpp" // the row search by time and the position within a step are the conflict call's

#if defined(__HIPCC__)
#define PPM_INLINE __host__ __device__ __forceinline__
#else
#define PPM_INLINE inline
#endif

namespace ppm {

/// a call lists no more stops per plan than this, and looks no more values up than that
constexpr int kMaxStops = 1 << 16;
constexpr int64_t kMaxLookups = (int64_t)1 << 26;

constexpr int kInside = 0, kBefore = 1, kBehind = 2;

/// what a look-up finds in the rows: pp_timetable_result without the pose and the next stop
struct Sample {
	int status, row;
	double s, t, v, a;
};

/// sample j is a stop iff it stands
PPM_INLINE bool is_stop(double v) { return v == 0.0; }

/// t_arrive of row j of a profile's (s, v, t) rows: 0 for row 0, else the time of the row before it plus the motion time of the step between them
/// (t_j itself has the dwell in it too)
PPM_INLINE double arrive_time(const double* rows, int j, double aAcc, double aDec)
{
	if (j == 0)
		return 0.0;
	const double* const r = rows + 3 * (size_t)(j - 1);
	return r[2] + ppv::step_time(r[3] - r[0], r[1], r[4], aAcc, aDec);
}

/// The largest j in 0 .. N - 1 with s_j <= s, s_j = rows[3 j] the non-decreasing arc lengths of a profile's rows (s_0 <= s): behind equal arc
/// lengths the LAST row
PPM_INLINE int row_of_length(const double* rows, int N, double s)
{
	int lo = 0, hi = N - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (rows[3 * (size_t)mid] <= s)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

/// Speed and acceleration `delta` seconds into the step from (s0, v0) to (s1, v1): ppc::step_position's cases
PPM_INLINE void step_speed(double s0, double v0, double s1, double v1, double delta, double aAcc, double aDec, double& v, double& a)
{
	const double ds = s1 - s0;
	a = 0.0;
	if (ds == 0.0) {
		v = v0;
		return;
	}
	const double m = ppv::step_time(ds, v0, v1, aAcc, aDec);
	if (delta >= m) {
		v = v1;
		return;
	}
	if (v0 + v1 > 0.0) {
		a = (v1 - v0) / m;
		v = v0 + a * delta;
		return;
	}
	const double x = ds * aDec / (aAcc + aDec);
	const double ta = __builtin_sqrt(2.0 * x / aAcc);
	if (delta <= ta) {
		v = aAcc * delta;
		a = aAcc;
	} else {
		v = aDec * (m - delta);
		a = -aDec;
	}
}

/// The time `delta` into the step from (s0, v0) to (s1, v1), s1 > s0, at which the vehicle is sigma = s - s0 metres into it, with the speed and the
/// acceleration there: the inverse of ppc::step_position, clamped into [0, m]
PPM_INLINE double step_inverse(double s0, double v0, double s1, double v1, double sigma, double aAcc, double aDec, double& v, double& a)
{
	const double ds = s1 - s0;
	const double m = ppv::step_time(ds, v0, v1, aAcc, aDec);
	double delta;
	if (v0 + v1 > 0.0) {
		a = (v1 - v0) / m;
		if (sigma == 0.0) {
			delta = 0.0;
			v = v0;
		} else {
			double w = v0 * v0 + (2.0 * a) * sigma;
			if (!(w > 0.0))
				w = 0.0;
			v = __builtin_sqrt(w);
			delta = (2.0 * sigma) / (v0 + v);
		}
	} else {
		const double x = ds * aDec / (aAcc + aDec);
		if (sigma == 0.0) {
			delta = 0.0;
			v = v0;
			a = aAcc;
		} else if (sigma <= x) {
			delta = __builtin_sqrt(2.0 * sigma / aAcc);
			v = aAcc * delta;
			a = aAcc;
		} else {
			const double r = __builtin_sqrt(2.0 * (ds - sigma) / aDec);
			delta = m - r;
			v = aDec * r;
			a = -aDec;
		}
	}
	if (!(delta >= 0.0))
		delta = 0.0;
	if (delta > m)
		delta = m;
	return delta;
}

/// the look-up by time: u seconds after the start of a profile of N >= 1 rows
PPM_INLINE Sample at_time(const double* rows, int N, double u, double aAcc, double aDec)
{
	Sample q;
	const double end = rows[3 * (size_t)(N - 1) + 2];
	q.status = kInside;
	if (u < 0.0) {
		q.status = kBefore;
		u = 0.0;
	}
	if (u > end) {
		q.status = kBehind;
		u = end;
	}
	const int j = ppc::row_of(rows, N, u);
	const double* const r = rows + 3 * (size_t)j;
	q.row = j;
	q.t = u;
	if (j == N - 1) {
		q.s = r[0];
		q.v = r[1];
		q.a = 0.0;
		return q;
	}
	q.s = ppc::step_position(r[0], r[1], r[3], r[4], u - r[2], aAcc, aDec);
	step_speed(r[0], r[1], r[3], r[4], u - r[2], aAcc, aDec, q.v, q.a);
	return q;
}

/// the look-up by arc length: at s along a profile of N >= 1 rows
PPM_INLINE Sample at_length(const double* rows, int N, double s, double aAcc, double aDec)
{
	Sample q;
	const double first = rows[0], last = rows[3 * (size_t)(N - 1)];
	q.status = kInside;
	if (s < first) {
		q.status = kBefore;
		s = first;
	}
	if (s > last) {
		q.status = kBehind;
		s = last;
	}
	const int j = row_of_length(rows, N, s);
	const double* const r = rows + 3 * (size_t)j;
	q.row = j;
	q.s = s;
	if (j == N - 1) {
		q.t = r[2];
		q.v = r[1];
		q.a = 0.0;
		return q;
	}
	const double delta = step_inverse(r[0], r[1], r[3], r[4], s - r[0], aAcc, aDec, q.v, q.a);
	q.t = r[2] + delta;
	return q;
}

/// The first of `listed` stops, in row order, whose row is > j: its index, or -1.  The row of stop i is rowOf[i * stride] (a pp_timetable_stop
/// array seen as int32: stride 8).
PPM_INLINE int next_stop(const int32_t* rowOf, int stride, int listed, int j)
{
	int lo = 0, hi = listed; // the first i in 0 .. listed with row_i > j (listed: none)
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (rowOf[(size_t)mid * (size_t)stride] > j)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo < listed ? lo : -1;
}

} // namespace ppm
