// The sample schedule and the cell rule of a stamp (include/pp_hip.h, "stamping held plans into a map"), as k_stamp_tickets
// (pp_stamp.hpp) runs them and as a plain C++ program can run them: nothing here needs the device, a map or libm.  Integer and
// double arithmetic only, every expression written in the order the header defines it (the library is built without contraction;
// tests/cpp/test_stamp_rule.cpp is too), so host and device give the same bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PPS_INLINE __host__ __device__ __forceinline__
#else
#define PPS_INLINE inline
#endif

namespace pps {

/// steps of an edge are capped here (an edge of 5 m at 10 um): a plan's sample count stays inside an int32 for every path capacity
constexpr int kMaxSteps = 1 << 19;

/// n = L > 0 ? (int)ceil(L / spacing) : 0, in double; the edge has n + 1 samples (one for n == 0).  A NaN length gives 0.
PPS_INLINE int edge_steps(double L, double spacing)
{
	if (!(L > 0.0))
		return 0;
	const double q = L / spacing;
	if (!(q < (double)kMaxSteps))
		return kMaxSteps;
	int n = (int)q; // truncation: q > 0
	if ((double)n < q)
		n++;
	return n;
}

/// ratio of sample k of an edge of n steps: both ends are samples
PPS_INLINE double sample_ratio(int k, int n) { return n == 0 ? 0.0 : (double)k / (double)n; }

/// arc length of a sample: S_e = the sequential sum of the lengths of the edges before it
PPS_INLINE double sample_arc_length(double Se, double ratio, double L) { return Se + ratio * L; }

PPS_INLINE bool in_window(double s, double from, double to) { return s >= from && s <= to; }

/// the target's geometry: cell (row, col) spans [gx + row res, gx + (row + 1) res) x [gy + col res, gy + (col + 1) res)
struct Grid {
	int rows, cols;
	double res; // (double) of the map's float resolution
	double gx, gy;
};

PPS_INLINE double cell_centre(double origin, int index, double res) { return origin + ((double)index + 0.5) * res; }

/// Indices lo .. hi (inside 0 .. n - 1; lo > hi: none) that hold every cell of one axis whose centre can lie within R of c: the cell
/// of c - R less one to the cell of c + R plus one, clipped in double BEFORE the conversion, so that a coordinate far outside the grid,
/// an infinite one or a NaN (an empty range) never reaches an integer conversion it does not fit.  The spare cell on either side
/// makes the rounding of the quotient irrelevant: which cells are covered is decided by covers() alone.
PPS_INLINE void axis_range(double c, double R, double origin, double res, int n, int& lo, int& hi)
{
	const double a = ((c - R) - origin) / res - 1.0, b = ((c + R) - origin) / res + 1.0;
	lo = a > 0.0 ? (a < (double)n ? (int)a : n) : 0;
	hi = b < (double)n ? (b >= 0.0 ? (int)b : -1) : n - 1;
	if (!(a == a) || !(b == b)) {
		lo = 0;
		hi = -1;
	}
}

/// the cell is covered iff its centre satisfies dx^2 + dy^2 <= R^2
PPS_INLINE bool covers(const Grid& g, int row, int col, double cx, double cy, double R)
{
	const double dx = cell_centre(g.gx, row, g.res) - cx, dy = cell_centre(g.gy, col, g.res) - cy;
	return dx * dx + dy * dy <= R * R;
}

/// R_i = (double)r_i + (double)margin
PPS_INLINE double effective_radius(float r, float margin) { return (double)r + (double)margin; }

} // namespace pps
