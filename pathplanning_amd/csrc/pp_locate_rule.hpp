// The arithmetic of locating a vehicle on a plan (include/pp_hip.h, "locating vehicles on held plans"), as k_locate_tickets
// (pp_locate.hpp) runs it and as a plain C++ program can run it: the heading wrap, the cost of a path pose, the (c, s) order, the
// lattice of the second stage and the mapping arc length -> (edge, ratio) over an array of S_e.  Nothing here needs the device or a
// map; double arithmetic only, every expression written in the order the header defines it (the library is built without
// contraction; tests/cpp/test_locate_rule.cpp is too), so host and device give the same bits.  rint and floor are the compiler's
// builtins: one instruction on either side, exact by definition.
#pragma once
#include <cstdint>

#include "pp_stamp_rule.hpp" // the sample schedule and pps::in_window are the stamp's

#if defined(__HIPCC__)
#define PPL_INLINE __host__ __device__ __forceinline__
#else
#define PPL_INLINE inline
#endif

namespace ppl {

constexpr double kTwoPi = 6.283185307179586;
/// the second stage looks at lattice points i0 - kLatticeBelow .. i0 + kLatticeAbove of the lattice i * (spacing / kLatticePerSpacing)
constexpr int kLatticePerSpacing = 32, kLatticeBelow = 32, kLatticeAbove = 33, kLatticePoints = kLatticeBelow + kLatticeAbove + 1;

/// d = a - TWO_PI * rint(a / TWO_PI): the heading difference a brought to [-pi, pi] (ties of rint to even)
PPL_INLINE double wrap(double a) { return a - kTwoPi * __builtin_rint(a / kTwoPi); }

/// what the vehicle V sees of a path pose P
struct Error {
	double ex, ey, dtheta;
};
PPL_INLINE Error error_of(double vx, double vy, double vt, double px, double py, double pt) { return Error { vx - px, vy - py, wrap(vt - pt) }; }

/// c = (ex ex + ey ey) + (w dtheta)(w dtheta), metres squared
PPL_INLINE double cost(const Error& e, double w) { return (e.ex * e.ex + e.ey * e.ey) + (w * e.dtheta) * (w * e.dtheta); }

/// the order of candidates: the smaller c, on equal c the smaller s
PPL_INLINE bool better(double c, double s, double cBest, double sBest) { return c < cBest || (c == cBest && s < sBest); }

/// Sample k of the n steps of edge `edge` is the end of an edge that has a successor: the junction pose, which the successor's sample 0 names
/// (one point of the plan gets one (edge, ratio): the later edge at ratio 0, as edge_of() gives a lattice point that falls on S_e)
PPL_INLINE bool names_next_edge(int k, int n, int edge, int nEdges) { return n > 0 && k == n && edge < nEdges; }

/// delta = spacing / 32
PPL_INLINE double lattice_step(double spacing) { return spacing / (double)kLatticePerSpacing; }

/// i0 - 32 with i0 = (int64) floor(s1 / delta): the first of the kLatticePoints lattice indices.  The quotient is clipped in double BEFORE
/// the conversion (a step that underflowed to zero, or a spacing of 1e-300, never reaches a conversion it does not fit).
PPL_INLINE int64_t lattice_first(double s1, double delta)
{
	double q = __builtin_floor(s1 / delta);
	if (!(q < 4611686018427387904.0)) // 2^62; a NaN too
		q = 4611686018427387904.0;
	if (q < -4611686018427387904.0)
		q = -4611686018427387904.0;
	return (int64_t)q - kLatticeBelow;
}

/// lattice point i: u = (double)i * delta, a candidate iff 0 <= u <= length and pps::in_window(u, from, to)
PPL_INLINE bool lattice_point(int64_t i, double delta, double length, double from, double to, double& u)
{
	u = (double)i * delta;
	return u >= 0.0 && u <= length && pps::in_window(u, from, to);
}

/// The largest e in 1 .. nEdges with S_e <= u, S[e - 1] = S_e the non-decreasing sums (S_1 = 0 <= u): behind zero-length edges the LAST
/// edge that starts at u, and for u equal to an S_e edge e at ratio 0, not edge e - 1 at ratio 1.
PPL_INLINE int edge_of(const double* S, int nEdges, double u)
{
	int lo = 1, hi = nEdges;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (S[mid - 1] <= u)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

/// ratio = L_e > 0 ? (u - S_e) / L_e : 0, capped at 1
PPL_INLINE double ratio_of(double u, double Se, double Le)
{
	if (!(Le > 0.0))
		return 0.0;
	const double r = (u - Se) / Le;
	return r > 1.0 ? 1.0 : r;
}

} // namespace ppl
