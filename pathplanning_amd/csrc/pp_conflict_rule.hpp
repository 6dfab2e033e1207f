// The arithmetic of space-time conflicts between held plans (include/pp_hip.h, "space-time conflicts between held plans"), as
// k_trajectory_tickets and k_conflict_pairs (pp_conflicts.hpp) run it and as a plain C++ program can run it: the global time lattice,
// the search of a profile's rows for a time, the position within a step of the profile, the separation of two discs, and the two
// orders of the pair record.  Nothing here needs the device or a map; double arithmetic only, every expression written in the order
// the header defines it (the library is built without contraction; tests/cpp/test_conflict_rule.cpp is too), so host and device give
// the same bits.  The only library function is the square root, the compiler's builtin: correctly rounded on either side.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pp_speed_rule.hpp" // the time of a step is the speed profile's

#if defined(__HIPCC__)
#define PPC_INLINE __host__ __device__ __forceinline__
#else
#define PPC_INLINE inline
#endif

namespace ppc {

/// a call looks at no more lattice times than this
constexpr int64_t kMaxTimes = 1 << 20;

/// a quotient of doubles as a lattice index: clipped to +-2^62 in double BEFORE the conversion, as ppl::lattice_first does (a NaN: 2^62)
PPC_INLINE int64_t lattice_index(double q)
{
	if (!(q < 4611686018427387904.0))
		q = 4611686018427387904.0;
	if (q < -4611686018427387904.0)
		q = -4611686018427387904.0;
	return (int64_t)q;
}
/// k0 = (int64) ceil(t_from / dt), k1 = (int64) floor(t_to / dt)
PPC_INLINE int64_t lattice_begin(double tFrom, double dt) { return lattice_index(__builtin_ceil(tFrom / dt)); }
PPC_INLINE int64_t lattice_end(double tTo, double dt) { return lattice_index(__builtin_floor(tTo / dt)); }
/// T = k1 - k0 + 1, formed without overflow: 0 for k1 < k0, and kMaxTimes + 1 for everything above kMaxTimes
PPC_INLINE int64_t lattice_count(int64_t k0, int64_t k1)
{
	if (k1 < k0)
		return 0;
	const uint64_t d = (uint64_t)k1 - (uint64_t)k0;
	return d >= (uint64_t)kMaxTimes ? kMaxTimes + 1 : (int64_t)d + 1;
}
/// tau_m = (double)(k0 + m) * dt: the lattice is global, not anchored at t_from
PPC_INLINE double lattice_time(int64_t k0, int64_t m, double dt) { return (double)(k0 + m) * dt; }

/// The largest j in 0 .. N - 1 with t_j <= u, t_j = rows[3 j + 2] the non-decreasing times of a profile's (s, v, t) rows (t_0 = 0 <= u):
/// behind equal times the LAST row
PPC_INLINE int row_of(const double* rows, int N, double u)
{
	int lo = 0, hi = N - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (rows[3 * (size_t)mid + 2] <= u)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

/// The arc length `delta` seconds into the step from (s0, v0) to (s1, v1): the standstill of a step without length, the dwell behind the
/// step's motion time, the trapezoid's constant acceleration, or the two halves of step_time's triangle; clamped into [s0, s1]
PPC_INLINE double step_position(double s0, double v0, double s1, double v1, double delta, double aAcc, double aDec)
{
	const double ds = s1 - s0;
	if (ds == 0.0)
		return s0;
	const double m = ppv::step_time(ds, v0, v1, aAcc, aDec);
	if (delta >= m)
		return s1;
	double s;
	if (v0 + v1 > 0.0) {
		const double a = (v1 - v0) / m;
		s = s0 + (v0 + (0.5 * a) * delta) * delta;
	} else {
		const double x = ds * aDec / (aAcc + aDec);
		const double ta = __builtin_sqrt(2.0 * x / aAcc);
		if (delta <= ta)
			s = s0 + (0.5 * aAcc) * delta * delta;
		else {
			const double r = m - delta;
			s = s1 - (0.5 * aDec) * r * r;
		}
	}
	if (s < s0)
		s = s0;
	if (s > s1)
		s = s1;
	return s;
}

/// Where the vehicle of a profile (N >= 1 rows) is u = tau - t_start seconds after its start: false if it is absent (before its start
/// without hold_before, behind its last row's time without hold_after), else its arc length
PPC_INLINE bool position(const double* rows, int N, double u, double aAcc, double aDec, int holdBefore, int holdAfter, double& s)
{
	if (u < 0.0) {
		s = rows[0];
		return holdBefore != 0;
	}
	if (u > rows[3 * (size_t)(N - 1) + 2]) {
		s = rows[3 * (size_t)(N - 1)];
		return holdAfter != 0;
	}
	const int j = row_of(rows, N, u);
	const double* const r = rows + 3 * (size_t)j;
	if (j == N - 1) {
		s = r[0];
		return true;
	}
	s = step_position(r[0], r[1], r[3], r[4], u - r[2], aAcc, aDec);
	return true;
}

/// The p-th pair (i, j), i < j < n, of the row-major list of all of them (0 <= p < n (n - 1) / 2): row i starts at i (2 n - i - 1) / 2, and i is
/// the last row that starts at or before p
PPC_INLINE void pair_of(int n, int64_t p, int& i, int& j)
{
	int lo = 0, hi = n - 2;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if ((int64_t)mid * (2 * (int64_t)n - mid - 1) / 2 <= p)
			lo = mid;
		else
			hi = mid - 1;
	}
	i = lo;
	j = (int)(p - (int64_t)lo * (2 * (int64_t)n - lo - 1) / 2) + lo + 1;
}

/// the separation of two discs whose centres are (dx, dy) apart
PPC_INLINE double separation(double dx, double dy, double Ra, double Rb) { return __builtin_sqrt(dx * dx + dy * dy) - (Ra + Rb); }
PPC_INLINE bool in_conflict(double sep, double margin) { return sep < margin; }

/// the order of candidates for min_separation: the smaller separation, on equal separations the smaller tau
PPC_INLINE bool closer(double sep, double tau, double sepBest, double tauBest) { return sep < sepBest || (sep == sepBest && tau < tauBest); }
/// the order of conflicts: the smaller tau
PPC_INLINE bool earlier(double tau, double tauBest) { return tau < tauBest; }

} // namespace ppc
