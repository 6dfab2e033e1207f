// The rule of the space-time broad phase (include/pp_hip.h, "the pairs that can meet"), as k_plan_boxes and k_box_pairs (pp_pairs.hpp) and the
// host side of the call (pp_planner.hip) run it and as a plain C++ program can run it: how many boxes a lattice has, which columns of a plan's
// extended trajectory a box covers, the reach of two vehicles, the bounding box as something points are put into and boxes are merged into, and the
// two-axis test of two boxes.  Double arithmetic only, every expression in the order the header defines it (the library is built without
// contraction; tests/cpp/test_pair_rule.cpp is too).  The only library function is the square root, the compiler's builtin: correctly rounded on
// either side.  No allocation: the caller brings every array.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PPB_INLINE __host__ __device__ __forceinline__
#else
#define PPB_INLINE inline
#endif

namespace ppb {

/// B is 1 .. kMaxTimesPerBox, and a call forms at most kMaxBoxes boxes (n * NB)
constexpr int64_t kMaxTimesPerBox = 1 << 20;
constexpr int64_t kMaxBoxes = 1 << 26;

/// NB = ceil(T / B)
PPB_INLINE int64_t box_count(int64_t T, int64_t B) { return (T + B - 1) / B; }

/// Box b covers the lattice times b B .. min(b B + B, T) - 1.  Under a delay d in 0 .. D such a time m reads column m + D - d of the extended trajectory
/// (ppy::column), so the box covers the columns first_column .. last_column, both inside 0 .. T + D - 1
PPB_INLINE int64_t first_column(int64_t b, int64_t B) { return b * B; }
PPB_INLINE int64_t last_column(int64_t b, int64_t B, int64_t T, int64_t D)
{
	const int64_t end = b * B + B;
	return (end < T ? end : T) - 1 + D;
}

/// how far a disc (ox, oy, r) reaches from the reference point
PPB_INLINE double disc_reach(double ox, double oy, double r) { return __builtin_sqrt(ox * ox + oy * oy) + r; }
/// reach = (margin + (R + R)) + 1e-6, R the largest disc_reach of the footprint: two vehicles whose reference points are further apart than this on
/// one axis have no two discs closer than the margin; the micrometre covers the rounding of the narrow phase for coordinates below 10^6 m
PPB_INLINE double reach(double margin, double R) { return (margin + (R + R)) + 1e-6; }

/// (xmin, ymin, xmax, ymax) of the reference point over the columns a plan is present at; four NaNs: present at none
struct Box {
	double xmin, ymin, xmax, ymax;
};
PPB_INLINE Box no_box()
{
	const double none = __builtin_nan("");
	return Box { none, none, none, none };
}
PPB_INLINE bool exists(const Box& a) { return a.xmin == a.xmin; }

/// a becomes the box of a and o: only min and max are formed, so the order in which points and boxes arrive does not matter
PPB_INLINE void merge(Box& a, const Box& o)
{
	if (!exists(o))
		return;
	if (!(a.xmin <= o.xmin))
		a.xmin = o.xmin;
	if (!(a.ymin <= o.ymin))
		a.ymin = o.ymin;
	if (!(a.xmax >= o.xmax))
		a.xmax = o.xmax;
	if (!(a.ymax >= o.ymax))
		a.ymax = o.ymax;
}
/// ... of a and the reference point (x, y) of one column; x is a NaN where the plan is absent
PPB_INLINE void accumulate(Box& a, double x, double y) { merge(a, Box { x, y, x, y }); }

/// the gap of two intervals on one axis: positive when they are apart
PPB_INLINE double gap(double minA, double maxA, double minB, double maxB)
{
	const double ab = minA - maxB, ba = minB - maxA;
	return ab > ba ? ab : ba;
}
/// Can plans with these boxes of one block of lattice times have discs closer than the margin there?  Both boxes exist, and on neither axis is the gap
/// larger than the reach
PPB_INLINE bool can_meet(const Box& a, const Box& b, double reach)
{
	if (!exists(a) || !exists(b))
		return false;
	const double gx = gap(a.xmin, a.xmax, b.xmin, b.xmax), gy = gap(a.ymin, a.ymax, b.ymin, b.ymax);
	return !(gx > reach) && !(gy > reach);
}

} // namespace ppb
