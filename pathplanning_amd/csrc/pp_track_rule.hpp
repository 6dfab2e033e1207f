// The rule of tracked movers in a delay call (include/pp_hip.h, "start delays that clear conflicts and tracked movers"), as k_track_samples,
// k_delay_level_tracks and k_track_pairs (pp_tracks.hpp) and the host side of the call (pp_planner.hip) run it and as a plain C++ program can run
// it: the search of a track's waypoints for a time, the track's position there, the partner index under which a track enters the key of a conflict
// (and its inverse), and the validation of a track set, which says what is wrong and where.  Double and integer arithmetic only, every expression
// written in the order the header defines it (the library is built without contraction; tests/cpp/test_track_rule.cpp is too), so host and device
// give the same bits.  No library function, no allocation: the caller brings every array.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pp_delay_rule.hpp" // the key is the delay call's, over n + M partners

#if defined(__HIPCC__)
#define PPK_INLINE __host__ __device__ __forceinline__
#else
#define PPK_INLINE inline
#endif

namespace ppk {

/// a call takes no more tracks, waypoint rows and (track, lattice time) samples than these
constexpr int64_t kMaxTracks = 1 << 16;
constexpr int64_t kMaxWaypoints = 1 << 24;
constexpr int64_t kMaxSamples = 1 << 26;

/// The largest j in 0 .. W - 1 with t_j <= tau, t_j = waypoints[3 j] the strictly increasing times of a track's (t, x, y) rows (t_0 <= tau)
PPK_INLINE int waypoint_of(const double* waypoints, int W, double tau)
{
	int lo = 0, hi = W - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (waypoints[3 * (size_t)mid] <= tau)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

/// Where the track of W >= 1 waypoint rows is at time tau: false if it is absent (before its first waypoint's time or behind its last one's),
/// else the waypoint itself at the last row, and between two rows the straight line at lam = (tau - t_j) / (t_{j+1} - t_j)
PPK_INLINE bool position(const double* waypoints, int W, double tau, double& x, double& y)
{
	if (tau < waypoints[0] || tau > waypoints[3 * (size_t)(W - 1)])
		return false;
	const int j = waypoint_of(waypoints, W, tau);
	const double* const r = waypoints + 3 * (size_t)j;
	if (j == W - 1) {
		x = r[1];
		y = r[2];
		return true;
	}
	const double lam = (tau - r[0]) / (r[3] - r[0]);
	x = r[1] + lam * (r[4] - r[1]);
	y = r[2] + lam * (r[5] - r[2]);
	return true;
}

/// In the key order of a candidate's conflicts track k of M is partner n + k behind the call's n vehicles: key = m * (n + M) + partner
PPK_INLINE int64_t partner_of_track(int64_t n, int64_t k) { return n + k; }
PPK_INLINE bool is_track(int64_t n, int64_t partner) { return partner >= n; }
PPK_INLINE int64_t track_of_partner(int64_t n, int64_t partner) { return partner - n; }
PPK_INLINE uint64_t key(int64_t m, int64_t n, int64_t M, int64_t partner) { return ppy::key(m, n + M, partner); }
PPK_INLINE int32_t time_of(uint64_t key, int64_t n, int64_t M) { return ppy::time_of(key, n + M); }
PPK_INLINE int32_t partner_of(uint64_t key, int64_t n, int64_t M) { return ppy::partner_of(key, n + M); }

/// (x - x is zero for every finite x and a NaN for the rest)
PPK_INLINE bool finite(double x) { return x - x == 0.0; }

/// what validate() found, in the order it looks
enum Fault : int32_t {
	kValid = 0,
	kReserved,        // reserved != 0
	kCount,           // M < 0 or M > kMaxTracks
	kNullOffsets,     // M > 0 and no offsets
	kNullWaypoints,   // M > 0 and no waypoints
	kNullRadii,       // M > 0 and no radii
	kFirstOffset,     // offsets[0] != 0
	kOffsetOrder,     // offsets[index + 1] <= offsets[index]: track `index` owns no row
	kWaypointCount,   // offsets[M] > kMaxWaypoints
	kSampleCount,     // M * T > kMaxSamples
	kWaypointValue,   // waypoint row `index` (of track `track`) holds a value that is not finite
	kWaypointOrder,   // waypoint row `index` (of track `track`) has a time that is not above the row's before it
	kRadius,          // radii[index] is not finite and >= 0
};
struct Verdict {
	Fault fault;
	int64_t index; // the first offender: a track, or a waypoint row counted over the whole set
	int64_t track; // the track a waypoint row belongs to; else -1
};

/// Is this a track set a call over T lattice times takes?  The first thing wrong, in the order of Fault; reads nothing behind a fault.
inline Verdict validate(int32_t M, int32_t reserved, const int32_t* offsets, const double* waypoints, const double* radii, int64_t T)
{
	if (reserved != 0)
		return { kReserved, -1, -1 };
	if (M < 0 || M > kMaxTracks)
		return { kCount, -1, -1 };
	if (M == 0)
		return { kValid, -1, -1 };
	if (!offsets)
		return { kNullOffsets, -1, -1 };
	if (!waypoints)
		return { kNullWaypoints, -1, -1 };
	if (!radii)
		return { kNullRadii, -1, -1 };
	if (offsets[0] != 0)
		return { kFirstOffset, 0, -1 };
	for (int32_t k = 0; k < M; k++)
		if (offsets[k + 1] <= offsets[k])
			return { kOffsetOrder, k, -1 };
	if (offsets[M] > kMaxWaypoints)
		return { kWaypointCount, -1, -1 };
	if ((int64_t)M * T > kMaxSamples)
		return { kSampleCount, -1, -1 };
	for (int32_t k = 0; k < M; k++)
		for (int64_t r = offsets[k]; r < offsets[k + 1]; r++) {
			const double* const w = waypoints + 3 * (size_t)r;
			if (!finite(w[0]) || !finite(w[1]) || !finite(w[2]))
				return { kWaypointValue, r, k };
			if (r > offsets[k] && !(w[0] > w[-3]))
				return { kWaypointOrder, r, k };
		}
	for (int32_t k = 0; k < M; k++)
		if (!finite(radii[k]) || !(radii[k] >= 0.0))
			return { kRadius, k, -1 };
	return { kValid, -1, -1 };
}

} // namespace ppk
