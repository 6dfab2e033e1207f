// Vehicle footprint on the device: the pose's validity against K discs fixed in the vehicle frame instead of the one
// look-up at the reference point (pp_device.hpp: is_state_valid), and the adaptive march of is_path_valid over it.
// The definition (include/pp_hip.h, "vehicle footprint") is restated here line by line; the numpy restatement the
// tests compare against is tests/footprint_ref.py.  gfx950 only, -ffp-contract=off like everything in this directory.
#pragma once

#include "pp_device.hpp"

namespace ppd {

constexpr int kFootprintMaxDiscs = 8;

/// A footprint as a kernel argument (passed by value: wave-uniform, so it lives in SGPRs).  Disc i has its centre at
/// (ox, oy) in the vehicle frame (origin = the pose's reference point, x forward, y left) and radius r.
struct Footprint {
	int n;          // discs in use, 1..8
	int anyOffset;  // some disc has (ox, oy) != (0, 0): the pose's sin / cos are needed
	double rho;     // max_i hypot(ox_i, oy_i): how far a disc centre sits from the reference point
	double ox[kFootprintMaxDiscs], oy[kFootprintMaxDiscs];
	float r[kFootprintMaxDiscs];
	int slot[kFootprintMaxDiscs]; // which of the footprint's validity bitmaps (one per distinct radius) holds disc i's comparison
};

/// disc centre in the world: the parentheses are part of the definition (no contraction, this order)
PPD_INLINE void disc_centre(const Footprint& fp, int i, double x, double y, double s, double c, double& cx, double& cy)
{
	if (fp.ox[i] == 0.0 && fp.oy[i] == 0.0) {
		cx = x;
		cy = y;
	} else {
		cx = (x + fp.ox[i] * c) - fp.oy[i] * s;
		cy = (y + fp.ox[i] * s) + fp.oy[i] * c;
	}
}

PPD_INLINE double dmin4(double r, double a, double b, double c, double d)
{
	if (a < r)
		r = a;
	if (b < r)
		r = b;
	if (c < r)
		r = c;
	if (d < r)
		r = d;
	return r;
}

/// State check of a pose against a footprint when sin / cos of its (unwrapped) heading are known.
///  1. the reference point passes everything is_state_valid tests except the distance comparison;
///  2. every disc centre lies inside the position bounds and the grid, and the cell's obstacle distance d_i >= r_i;
///  3. clearance = min_i (d_i - r_i); border = (float) min over the reference point and every centre of the four
///     distances to the position bounds (double min, one conversion, as fmin4).
/// clearance and border are defined only when the pose is valid.
PPD_INLINE bool fp_state_valid_sc(const MapView& m, const Footprint& fp, double x, double y, double theta, double s, double c, float& clearance, float& border)
{
	const double lx = x - m.lox, ly = y - m.loy;
	const double lt = wrap_theta(theta);
	int row, col;
	world_to_cell(m, x, y, row, col);
	if (lx < m.lbx || lx > m.ubx)
		return false;
	if (ly < m.lby || ly > m.uby)
		return false;
	if (lt < m.lbt || lt > m.ubt)
		return false;
	if (!inside_map(m, row, col))
		return false;
	double b = dmin4(x - m.lbx, m.ubx - x, y - m.lby, m.uby - y, __builtin_huge_val());
	float clear = __builtin_huge_valf();
	for (int i = 0; i < fp.n; i++) {
		double cx, cy;
		disc_centre(fp, i, x, y, s, c, cx, cy);
		const double lcx = cx - m.lox, lcy = cy - m.loy;
		if (!(lcx >= m.lbx && lcx <= m.ubx && lcy >= m.lby && lcy <= m.uby))
			return false;
		world_to_cell(m, cx, cy, row, col);
		if (!inside_map(m, row, col))
			return false;
		const float d = m.dist[(size_t)row * m.cols + col];
		if (!(d >= fp.r[i]))
			return false;
		clear = fminf(clear, d - fp.r[i]);
		b = dmin4(b, cx - m.lbx, m.ubx - cx, cy - m.lby, m.uby - cy);
	}
	clearance = clear;
	border = (float)b;
	return true;
}

/// fp_state_valid_sc in two halves (see is_state_valid_issue), so that the caller can put other work between the loads and their first
/// use: `issue` does every bounds test and starts the discs' distance loads (raw[i] for disc i < fp.n; a centre that fails its tests reads
/// cell 0 instead, so every load is in range), `finish` is the comparisons and the clearance.  Same verdict and, for a valid pose, the same
/// clearance as fp_state_valid_sc (a minimum in another order over the same floats); no border.  The loops are unrolled so that raw[]
/// stays in registers; fp.n is wave-uniform.
PPD_INLINE bool fp_state_valid_issue_sc(const MapView& m, const Footprint& fp, double x, double y, double theta, double s, double c, float (&raw)[kFootprintMaxDiscs])
{
	const double lx = x - m.lox, ly = y - m.loy;
	const double lt = wrap_theta(theta);
	int row, col;
	world_to_cell(m, x, y, row, col);
	bool in = !(lx < m.lbx || lx > m.ubx) && !(ly < m.lby || ly > m.uby) && !(lt < m.lbt || lt > m.ubt) && inside_map(m, row, col);
#pragma unroll
	for (int i = 0; i < kFootprintMaxDiscs; i++) {
		raw[i] = 0.0f;
		if (i < fp.n) {
			double cx, cy;
			disc_centre(fp, i, x, y, s, c, cx, cy);
			const double lcx = cx - m.lox, lcy = cy - m.loy;
			world_to_cell(m, cx, cy, row, col);
			const bool inside = lcx >= m.lbx && lcx <= m.ubx && lcy >= m.lby && lcy <= m.uby && inside_map(m, row, col);
			in = in && inside;
			raw[i] = m.dist[inside ? (size_t)row * m.cols + col : (size_t)0];
		}
	}
	return in;
}
PPD_INLINE bool fp_state_valid_finish(const Footprint& fp, bool inBounds, const float (&raw)[kFootprintMaxDiscs], float& clearance)
{
	float clear = __builtin_huge_valf();
#pragma unroll
	for (int i = 0; i < kFootprintMaxDiscs; i++)
		if (i < fp.n) {
			inBounds = inBounds && raw[i] >= fp.r[i];
			clear = fminf(clear, raw[i] - fp.r[i]);
		}
	clearance = clear;
	return inBounds;
}

/// the same with one sincos of the unwrapped heading, and none when every disc sits on the reference point
PPD_INLINE bool fp_state_valid(const MapView& m, const Footprint& fp, double x, double y, double theta, float& clearance, float& border)
{
	double s = 0.0, c = 1.0;
	if (fp.anyOffset)
		sincos(theta, &s, &c);
	return fp_state_valid_sc(m, fp, x, y, theta, s, c, clearance, border);
}

/// The verdict alone from the footprint's validity bitmaps (bit (row * cols + col) of bitmap fp.slot[i]: dist >= r_i, the
/// identical float comparison), without early exits: see is_state_valid_bit_flat.  `bits` is the footprint's bitmaps in
/// global memory, `wordsPer` 32-bit words apart.
template <typename Bits>
PPD_INLINE bool fp_state_valid_bits_flat(const MapView& m, const Footprint& fp, double x, double y, double theta, Bits bits, uint32_t wordsPer)
{
	const double lx = x - m.lox, ly = y - m.loy;
	double lt = theta;
	if (fabs(theta) > kPi)
		lt = wrap_theta(theta);
	const double qx = div_by(x - m.gx, (double)m.res, m.invRes), qy = div_by(y - m.gy, (double)m.res, m.invRes);
	const bool inRange = qx > -2147483649.0 && qx < 2147483648.0 && qy > -2147483649.0 && qy < 2147483648.0; // false for NaN
	bool ok = !(lx < m.lbx) & !(lx > m.ubx) & !(ly < m.lby) & !(ly > m.uby) & !(lt < m.lbt) & !(lt > m.ubt);
	ok &= inRange & ((unsigned)(int)qx < (unsigned)m.rows) & ((unsigned)(int)qy < (unsigned)m.cols);
	double s = 0.0, c = 1.0;
	if (fp.anyOffset)
		sincos(theta, &s, &c);
	for (int i = 0; i < fp.n; i++) { // wave-uniform trip count
		double cx, cy;
		disc_centre(fp, i, x, y, s, c, cx, cy);
		const double lcx = cx - m.lox, lcy = cy - m.loy;
		const double cqx = div_by(cx - m.gx, (double)m.res, m.invRes), cqy = div_by(cy - m.gy, (double)m.res, m.invRes);
		const bool cRange = cqx > -2147483649.0 && cqx < 2147483648.0 && cqy > -2147483649.0 && cqy < 2147483648.0;
		const int row = (int)cqx, col = (int)cqy;
		const bool inb = (lcx >= m.lbx) & (lcx <= m.ubx) & (lcy >= m.lby) & (lcy <= m.uby); // false for NaN
		const bool inside = cRange & ((unsigned)row < (unsigned)m.rows) & ((unsigned)col < (unsigned)m.cols);
		const uint32_t cell = inside ? (uint32_t)row * (uint32_t)m.cols + (uint32_t)col : 0u; // always in range
		const uint32_t bit = (bits[(uint32_t)fp.slot[i] * wordsPer + (cell >> 5)] >> (cell & 31)) & 1u;
		ok &= inb & inside & (bit != 0u);
	}
	return ok;
}

/// (float)(1.0 + kappaMax * rho): a disc centre at distance rho from the reference point moves up to this much faster
/// than the reference point while the heading turns at kappaMax radians per metre, so the march divides its step by it.
PPD_INLINE float fp_gain(const Footprint& fp, double kappaMax) { return (float)(1.0 + kappaMax * fp.rho); }

/// The march of is_path_valid (state_validator_occupancy_map.cpp:28-71) over a footprint: the step comes from the
/// footprint's clearance instead of distance - minSafeRadius, divided by gain >= 1:
///   step = fmaxf(fminf(clearance, border) / gain, m.minInterp)
/// `last`, the zero-length case, the 2^22-sample give-up and the check counter are as in is_path_valid.
template <typename PathT>
PPD_INLINE bool is_path_valid_fp(const MapView& m, const Footprint& fp, float gain, const PathT& path, const Pose& init, float& last, int& checks)
{
	const double pathLength = path.length;
	float clearance = 0.0f, border = 0.0f;
	if (pathLength == 0.0) {
		last = 1.0f;
		checks++;
		return fp_state_valid(m, fp, init.x, init.y, init.t, clearance, border);
	}
	double lastValidLength = 0.0;
	double length = 0.0;
	while (length < pathLength) {
		if (checks > (1 << 22)) {
			last = (float)(lastValidLength / pathLength);
			return false;
		}
		Pose s = path.interpolate(length / pathLength);
		checks++;
		if (!fp_state_valid(m, fp, s.x, s.y, s.t, clearance, border)) {
			last = (float)(lastValidLength / pathLength);
			return false;
		}
		lastValidLength = length;
		const float deltaLength = fminf(clearance, border) / gain;
		length += (double)fmaxf(deltaLength, m.minInterp);
	}
	last = 1.0f;
	return true;
}

/// `border` of a pose alone (step 3 of the state check), for a pose whose clearance is already known
PPD_INLINE float fp_border_sc(const MapView& m, const Footprint& fp, double x, double y, double s, double c)
{
	double b = dmin4(x - m.lbx, m.ubx - x, y - m.lby, m.uby - y, __builtin_huge_val());
	for (int i = 0; i < fp.n; i++) {
		double cx, cy;
		disc_centre(fp, i, x, y, s, c, cx, cy);
		b = dmin4(b, cx - m.lbx, m.ubx - cx, cy - m.lby, m.uby - cy);
	}
	return (float)b;
}

/// The same march over a constant-steer arc whose start pose has been checked already (is_path_valid_from): firstClearance is the
/// footprint's clearance at the start pose, < 0 when that pose is invalid; sin / cos of every sample's heading come with the sample.
/// Counts the first sample like is_path_valid_fp.
template <typename SinCos>
PPD_INLINE bool is_arc_valid_fp_from(const MapView& m, const Footprint& fp, float gain, const ArcSCT<SinCos>& path, float firstClearance, float& last, int& checks)
{
	const double pathLength = path.length;
	if (pathLength == 0.0) {
		last = 1.0f;
		checks++;
		return !(firstClearance < 0.0f);
	}
	checks++;
	if (firstClearance < 0.0f) {
		last = 0.0f;
		return false;
	}
	double lastValidLength = 0.0;
	double length = 0.0;
	{
		const float border = fp_border_sc(m, fp, path.init.x, path.init.y, path.sinF, path.cosF);
		const float deltaLength = fminf(firstClearance, border) / gain;
		length += (double)fmaxf(deltaLength, m.minInterp);
	}
	while (length < pathLength) {
		if (checks > (1 << 22)) {
			last = (float)(lastValidLength / pathLength);
			return false;
		}
		double s, c;
		const Pose p = path.interpolate_sc(length / pathLength, s, c);
		checks++;
		float clearance, border;
		if (!fp_state_valid_sc(m, fp, p.x, p.y, p.t, s, c, clearance, border)) {
			last = (float)(lastValidLength / pathLength);
			return false;
		}
		lastValidLength = length;
		const float deltaLength = fminf(clearance, border) / gain;
		length += (double)fmaxf(deltaLength, m.minInterp);
	}
	last = 1.0f;
	return true;
}

} // namespace ppd
