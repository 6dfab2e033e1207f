// The arithmetic of a speed profile along a plan (include/pp_hip.h, "speed profiles along held plans"), as k_speed_profile_tickets
// (pp_speed_profile.hpp) runs it and as a plain C++ program can run it: the travel direction a sample counts with, the cusp predicate, the
// speed cap and its square, the two one-sided envelopes, the time of a step and the tie rule of the clearance minimum.  Nothing here
// needs the device or a map; double arithmetic only, every expression written in the order the header defines it (the library is built
// without contraction; tests/cpp/test_speed_rule.cpp is too), so host and device give the same bits.  The only library function is the
// square root, the compiler's builtin: correctly rounded on either side.
#pragma once
#include <cstdint>

#include "pp_stamp_rule.hpp" // the sample schedule and pps::in_window are the stamp's

#if defined(__HIPCC__)
#define PPV_INLINE __host__ __device__ __forceinline__
#else
#define PPV_INLINE inline
#endif

namespace ppv {

/// travel directions as the rule sees them
constexpr int kForward = 1, kReverse = -1, kNoDirection = 0;

/// what a call asks for (pp_speed_profile_params without the sample spacing)
struct Limits {
	double vMaxForward, vMaxReverse; // m/s
	double aAcc, aDec, aLat;         // m/s^2
	double dwell;                    // s, added at every cusp stop
	double clearanceGain, vFloor;    // 1/s and m/s: cap <= vFloor + clearanceGain * clearance; gain == 0: no clearance term
};

/// The direction sample j counts with: its own, or -- where its path object reports no motion -- its predecessor's in the sequence
/// (kNoDirection while no sample of the sequence has moved yet)
PPV_INLINE int carried_direction(int own, int previous) { return own == kNoDirection ? previous : own; }

/// sample j > 0 is a cusp stop iff it and its predecessor both travel and travel in different directions (directions as carried_direction gives them)
PPV_INLINE bool is_cusp(int direction, int previous) { return direction != kNoDirection && previous != kNoDirection && direction != previous; }

PPV_INLINE double min_of(double a, double b) { return b < a ? b : a; }

/// the speed cap of a sample: the direction's limit, the lateral-acceleration limit where the path is curved (kappa >= 0), the clearance limit where asked
PPV_INLINE double cap(const Limits& L, int direction, double kappa, float clearance)
{
	double c = direction == kForward ? L.vMaxForward : L.vMaxReverse;
	if (kappa > 0.0)
		c = min_of(c, __builtin_sqrt(L.aLat / kappa));
	if (L.clearanceGain > 0.0)
		c = min_of(c, L.vFloor + L.clearanceGain * (double)clearance);
	return c;
}

/// w: the cap squared, 0 at a cusp stop, then limited by the start speed at the first sample and by the end speed at the last (in this order when both)
PPV_INLINE double cap_squared(double c, bool cusp, bool first, bool last, double vStart, double vEnd)
{
	double w = c * c;
	if (cusp)
		w = 0.0;
	if (first)
		w = min_of(w, vStart * vStart);
	if (last)
		w = min_of(w, vEnd * vEnd);
	return w;
}

/// A_i = w_i - (2 a_acc) s_i; F_j = min_{i <= j} A_i; fwd_j = F_j + (2 a_acc) s_j: what accelerating from any earlier sample allows at j
PPV_INLINE double forward_key(double w, double s, double aAcc) { return w - (2.0 * aAcc) * s; }
PPV_INLINE double forward_limit(double F, double s, double aAcc) { return F + (2.0 * aAcc) * s; }
/// B_i = w_i + (2 a_dec) s_i; G_j = min_{i >= j} B_i; bwd_j = G_j - (2 a_dec) s_j: what braking for any later sample allows at j
PPV_INLINE double backward_key(double w, double s, double aDec) { return w + (2.0 * aDec) * s; }
PPV_INLINE double backward_limit(double G, double s, double aDec) { return G - (2.0 * aDec) * s; }

/// e_j = max(0, min(w_j, min(fwd_j, bwd_j))): the speed squared
PPV_INLINE double envelope(double w, double fwd, double bwd)
{
	const double m = min_of(w, min_of(fwd, bwd));
	return m > 0.0 ? m : 0.0;
}
PPV_INLINE double speed(double e) { return __builtin_sqrt(e); }

/// The time from a sample to the next one, ds = s1 - s0 >= 0 apart, with the speeds v0 and v1 at them: the trapezoid; where both stand and the
/// samples differ, the triangle that accelerates over x = ds a_dec / (a_acc + a_dec) and brakes over the rest
PPV_INLINE double step_time(double ds, double v0, double v1, double aAcc, double aDec)
{
	if (ds == 0.0)
		return 0.0;
	if (v0 + v1 > 0.0)
		return (2.0 * ds) / (v0 + v1);
	const double x = ds * aDec / (aAcc + aDec);
	return __builtin_sqrt(2.0 * x / aAcc) + __builtin_sqrt(2.0 * (ds - x) / aDec);
}

/// the record's clearance minimum: the smaller clearance, on equal clearances the smaller s
PPV_INLINE bool lower_clearance(double cl, double s, double clBest, double sBest) { return cl < clBest || (cl == clBest && s < sBest); }

} // namespace ppv
