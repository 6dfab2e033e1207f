// The rule of prioritised waits at stops on the conflicts lattice (include/pp_hip.h, "waits at stops that clear conflicts"), as k_wait_places and
// k_wait_level (pp_waits.hpp) and the host side of the call (pp_planner.hip) run it and as a plain C++ program can run it: the column at which a
// vehicle arrives at a stop, which column of its extended trajectory a lattice time reads under a wait (or that it stands at the stop), which stops
// are places, the order of the candidates and a candidate's ordinal, and the predicate of the exact shortcut.  Integer arithmetic, and the one
// double expression u_c = (double)(k0 - D + c) * dt - t_start in the order the header writes it; no library function, no allocation.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PPW_INLINE __host__ __device__ __forceinline__
#else
#define PPW_INLINE inline
#endif

namespace ppw {

/// a call lists no more places per vehicle than this
constexpr int kMaxPlaces = 1 << 10;

/// pp_wait_fixed::row and pp_wait_result::place: not decided by the caller / no wait; the start
constexpr int kFree = -2, kNoWait = -2, kStart = -1;

/// source(): the vehicle stands at the stop (no column of the trajectory)
constexpr int64_t kStanding = -1;

/// u_c: the time since the vehicle's start at column c of the extended trajectory, whose column 0 is lattice index kE = k0 - D
PPW_INLINE double since_start(int64_t kE, int64_t c, double dt, double tStart)
{
	const double tau = (double)(kE + c) * dt;
	return tau - tStart;
}

/// The arrive column of a stop: the smallest c in 0 .. columns - 1 with u_c >= tArrive, or `columns` if there is none (u_c never decreases in c)
PPW_INLINE int64_t arrive_column(int64_t kE, int64_t columns, double dt, double tStart, double tArrive)
{
	int64_t lo = 0, hi = columns; // the first c in 0 .. columns with u_c >= tArrive (columns: none)
	while (lo < hi) {
		const int64_t mid = lo + ((hi - lo) >> 1);
		if (since_start(kE, mid, dt, tStart) >= tArrive)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}

/// Where a vehicle that waits d steps (0 <= d) at the stop with arrive column a is at column c = m + D: a column of its extended trajectory, or
/// kStanding (present, at the stop's standing pose)
PPW_INLINE int64_t source(int64_t c, int64_t a, int64_t d)
{
	if (d == 0 || c < a)
		return c;
	return c < a + d ? kStanding : c - d;
}

/// ... and under a wait of d steps (0 <= d <= D) at the start: ppy::column(m, D, d) with c = m + D
PPW_INLINE int64_t source_start(int64_t c, int64_t d) { return c - d; }

/// a stop at `row` of a profile of N rows with arrive column a is a place of a free vehicle iff it is an inner row reached inside the horizon
PPW_INLINE bool is_place(int64_t row, int64_t N, int64_t a, int64_t D, int64_t columns) { return 0 < row && row < N - 1 && D <= a && a < columns; }

/// a fixed wait at `row` qualifies iff the row exists and stands and the vehicle gets there before the horizon ends
PPW_INLINE bool fixed_qualifies(int64_t row, int64_t N, bool stands, int64_t a, int64_t columns) { return 0 <= row && row < N && stands && a < columns; }

/// The candidates of a free vehicle with P listed places, S = 1 if it may wait at its start (else 0): ordinal 0 is d = 0; then for d = 1 .. D the
/// start (if S) and the places 0 .. P - 1
PPW_INLINE int64_t candidates(int64_t D, int64_t S, int64_t P) { return 1 + D * (S + P); }
/// the ordinal of the wait of d >= 1 steps at `place` (kStart, or 0 .. P - 1)
PPW_INLINE int64_t ordinal(int64_t place, int64_t d, int64_t S, int64_t P) { return 1 + (d - 1) * (S + P) + (place == kStart ? 0 : S + place); }
/// ... and back: the place (kNoWait for ordinal 0) and d of candidate o in 0 .. candidates() - 1
PPW_INLINE void candidate(int64_t o, int64_t S, int64_t P, int& place, int& d)
{
	if (o == 0) {
		place = kNoWait;
		d = 0;
		return;
	}
	const int64_t per = S + P, r = (o - 1) % per;
	d = (int)(1 + (o - 1) / per);
	place = S && r == 0 ? kStart : (int)(r - S);
}

/// The shortcut: if the d = 0 candidate's least key is at lattice time m0, a wait at a stop whose arrive column a is behind column m0 + D leaves
/// the vehicle where it was at every time up to m0, so the candidate is rejected with that same least key whatever its d
PPW_INLINE bool rejected_with_the_first(int64_t a, int64_t m0, int64_t D) { return a > m0 + D; }

} // namespace ppw
