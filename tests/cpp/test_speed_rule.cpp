// The arithmetic of a speed profile (pathplanning_amd/csrc/pp_speed_rule.hpp) run on the host: the same text k_speed_profile_tickets compiles for the
// device.  A stand-alone program, built with -fsanitize=address,undefined and without contraction by tests/test_speed_rule_host.py.  It checks
// itself (exit status 1 and a line on stderr at the first failure) and prints what it computed as hex floats, which the Python test compares with
// its numpy restatement bit for bit.
//   Q <name> <n> <a_acc> <a_dec> <v_start> <v_end>      a sequence follows
//   P <s> <cap> <cusp> <w> <e> <v> <t>                  one line per sample
//   T <ds> <v0> <v1> <a_acc> <a_dec> <step_time()>
//   D <own> <previous> <carried_direction()> / U <direction> <previous> <is_cusp()>
//   K <direction> <kappa> <clearance> <gain> <floor> <cap()>
// Checked here: the closed form (two one-sided envelopes) against a plain sequential forward-then-backward sweep, on hand-made sequences to 1e-12
// relative and on random ones to that plus the rounding of the keys (4 ulp of (2 a) s + w: see sequence()); the step between two standing samples;
// ds == 0; N == 1 with v_start and v_end; denormal and huge arc lengths.
#include "pp_speed_rule.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

uint64_t state = 0x2545F4914F6CDD1Dull;
uint64_t next()
{ // splitmix64
	uint64_t z = (state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(next() >> 11) * (1.0 / 9007199254740992.0); }

[[noreturn]] void fail(const char* what, const char* name, int j, double a, double b)
{
	std::fprintf(stderr, "FAILED %s: sequence %s, sample %d: %.17g against %.17g\n", what, name, j, a, b);
	std::exit(1);
}

const ppv::Limits kLimits { 5.0, 2.0, 1.5, 2.5, 2.0, 0.0, 0.0, 0.0 };

struct Profile {
	std::vector<double> w, e, v, t;
};

/// a sequence through the rule, as the kernel's passes run it: the keys' running minima from the front and from the back, then the times
Profile closed_form(const std::vector<double>& s, const std::vector<double>& cap, const std::vector<int>& cusp, const ppv::Limits& L, double vStart, double vEnd)
{
	const int n = (int)s.size();
	Profile p { std::vector<double>(n), std::vector<double>(n), std::vector<double>(n), std::vector<double>(n) };
	std::vector<double> fwd(n);
	double F = HUGE_VAL, G = HUGE_VAL;
	for (int j = 0; j < n; j++) {
		p.w[j] = ppv::cap_squared(cap[j], cusp[j] != 0, j == 0, j == n - 1, vStart, vEnd);
		F = ppv::min_of(F, ppv::forward_key(p.w[j], s[j], L.aAcc));
		fwd[j] = ppv::forward_limit(F, s[j], L.aAcc);
	}
	for (int j = n - 1; j >= 0; j--) {
		G = ppv::min_of(G, ppv::backward_key(p.w[j], s[j], L.aDec));
		p.e[j] = ppv::envelope(p.w[j], fwd[j], ppv::backward_limit(G, s[j], L.aDec));
		p.v[j] = ppv::speed(p.e[j]);
	}
	for (int j = 0; j + 1 < n; j++)
		p.t[j + 1] = p.t[j] + (ppv::step_time(s[j + 1] - s[j], p.v[j], p.v[j + 1], L.aAcc, L.aDec) + (cusp[j + 1] ? L.dwell : 0.0));
	return p;
}

/// the plain sweep: forward limited by acceleration from the predecessor, then backward limited by braking for the successor
std::vector<double> sweep(const std::vector<double>& s, const std::vector<double>& w, const ppv::Limits& L)
{
	const int n = (int)s.size();
	std::vector<double> e(w);
	for (int j = 1; j < n; j++)
		e[j] = std::fmin(e[j], e[j - 1] + 2.0 * L.aAcc * (s[j] - s[j - 1]));
	for (int j = n - 2; j >= 0; j--)
		e[j] = std::fmin(e[j], e[j + 1] + 2.0 * L.aDec * (s[j + 1] - s[j]));
	return e;
}

enum { kNone, kStrict, kKeys };

void sequence(const char* name, const std::vector<double>& s, const std::vector<double>& cap, const std::vector<int>& cusp, ppv::Limits L, double vStart, double vEnd, int compare)
{
	const int n = (int)s.size();
	const Profile p = closed_form(s, cap, cusp, L, vStart, vEnd);
	const std::vector<double> ref = sweep(s, p.w, L);
	std::printf("Q %s %d %a %a %a %a %a\n", name, n, L.aAcc, L.aDec, vStart, vEnd, L.dwell);
	for (int j = 0; j < n; j++) {
		std::printf("P %a %a %d %a %a %a %a\n", s[j], cap[j], cusp[j], p.w[j], p.e[j], p.v[j], p.t[j]);
		if (!(p.e[j] >= 0.0) || !std::isfinite(p.e[j]) || !std::isfinite(p.v[j]) || !std::isfinite(p.t[j]) || (j > 0 && p.t[j] < p.t[j - 1]))
			fail("a finite, non-negative profile with times that do not decrease", name, j, p.e[j], p.t[j]);
		if (p.e[j] > p.w[j])
			fail("e <= w", name, j, p.e[j], p.w[j]);
		if (cusp[j] && p.v[j] != 0.0)
			fail("standstill at a cusp stop", name, j, p.v[j], 0.0);
		// kStrict: 1e-12 relative.  kKeys: plus what the keys cost -- a key and its limit are each rounded once at the magnitude of (2 a) s_j + w, the sweep's
		// steps at the magnitude of e, so two results of exact arithmetic on the same w may differ by 4 * 2^-52 * ((2 a) s_j + max w) and no more
		double tolerance = 1e-12 * std::fmax(p.e[j], ref[j]);
		if (compare == kKeys)
			tolerance += 4.0 * 2.220446049250313e-16 * (2.0 * std::fmax(L.aAcc, L.aDec) * s[j] + 36.0);
		if (compare != kNone && std::fabs(p.e[j] - ref[j]) > tolerance)
			fail("closed form == sweep", name, j, p.e[j], ref[j]);
	}
	if (p.v[0] > vStart || p.v[n - 1] > vEnd)
		fail("the end speeds", name, 0, p.v[0], p.v[n - 1]);
}

void step(double ds, double v0, double v1, double aAcc, double aDec)
{
	const double dt = ppv::step_time(ds, v0, v1, aAcc, aDec);
	std::printf("T %a %a %a %a %a %a\n", ds, v0, v1, aAcc, aDec, dt);
	if (!(dt >= 0.0) || !std::isfinite(dt))
		fail("a finite step time >= 0", "step", 0, ds, dt);
}

} // namespace

int main()
{
	// ---- hand-made sequences
	{ // a straight run from rest to rest: accelerate, cruise, brake
		std::vector<double> s, cap;
		for (int j = 0; j <= 400; j++) {
			s.push_back(0.1 * j);
			cap.push_back(5.0);
		}
		sequence("rest-to-rest", s, cap, std::vector<int>(s.size(), 0), kLimits, 0.0, 0.0, kStrict);
	}
	{ // a slow bend in the middle, junctions sampled twice (ds == 0), a cusp stop with a dwell, a reverse leg
		std::vector<double> s, cap;
		std::vector<int> cusp;
		double at = 0.0;
		for (int edge = 0; edge < 12; edge++) {
			const bool reverse = edge >= 8, bend = edge == 3 || edge == 4;
			for (int k = 0; k <= 7; k++) {
				s.push_back(at + (double)k / 7.0 * 0.7);
				cap.push_back(reverse ? 2.0 : (bend ? std::sqrt(2.0 / 0.5) : 5.0));
				cusp.push_back(edge == 8 && k == 0);
			}
			at += 0.7;
		}
		ppv::Limits L = kLimits;
		L.dwell = 1.25;
		sequence("bend-cusp-reverse", s, cap, cusp, L, 1.0, 0.5, kStrict);
	}
	{ // N == 1: v_start first, then v_end
		sequence("one-a", { 0.0 }, { 5.0 }, { 0 }, kLimits, 3.0, 1.0, kStrict);
		sequence("one-b", { 7.5 }, { 5.0 }, { 0 }, kLimits, 1.0, 3.0, kStrict);
		sequence("one-c", { 0.0 }, { 0.5 }, { 0 }, kLimits, 3.0, 1.0, kStrict);
		const Profile a = closed_form({ 0.0 }, { 5.0 }, { 0 }, kLimits, 3.0, 1.0), c = closed_form({ 0.0 }, { 0.5 }, { 0 }, kLimits, 3.0, 1.0);
		if (a.v[0] != 1.0 || c.v[0] != 0.5)
			fail("N == 1 takes the least of cap, v_start and v_end", "one", 0, a.v[0], c.v[0]);
	}
	{ // two samples that both stand: the triangle
		sequence("two-standing", { 0.0, 2.0 }, { 5.0, 5.0 }, { 0, 0 }, kLimits, 0.0, 0.0, kStrict);
		const double dt = ppv::step_time(2.0, 0.0, 0.0, 1.5, 2.5), x = 2.0 * 2.5 / 4.0;
		if (std::fabs(dt - (std::sqrt(2.0 * x / 1.5) + std::sqrt(2.0 * (2.0 - x) / 2.5))) > 1e-15 || !(dt > 0.0))
			fail("the step between two standing samples", "two-standing", 0, dt, 0.0);
		// the triangle's peak speed is the same from both sides: a_acc x == a_dec (ds - x)
		if (std::fabs(1.5 * x - 2.5 * (2.0 - x)) > 1e-15)
			fail("the triangle's peak", "two-standing", 0, 1.5 * x, 2.5 * (2.0 - x));
	}
	// ---- random sequences: caps between 0.2 and 6 m/s, steps between 1 cm and 0.5 m, some repeated arc lengths, some cusp stops
	for (int r = 0; r < 40; r++) {
		const int n = 2 + (int)(next() % 300);
		std::vector<double> s, cap;
		std::vector<int> cusp;
		double at = uniform(0.0, 50.0);
		for (int j = 0; j < n; j++) {
			if (j > 0 && next() % 8 != 0)
				at += uniform(0.01, 0.5);
			s.push_back(at);
			cap.push_back(uniform(0.2, 6.0));
			cusp.push_back(j > 0 && next() % 37 == 0);
		}
		ppv::Limits L = kLimits;
		L.aAcc = uniform(0.3, 3.0);
		L.aDec = uniform(0.3, 4.0);
		L.dwell = r % 2 ? 0.0 : 0.75;
		char name[32];
		std::snprintf(name, sizeof name, "random-%d", r);
		sequence(name, s, cap, cusp, L, uniform(0.0, 3.0), r % 3 ? 0.0 : uniform(0.0, 3.0), kKeys);
	}
	// ---- denormal and huge arc lengths: no comparison with the sweep (the keys cancel there), only what must hold everywhere
	sequence("denormal", { 0.0, 4.9e-324, 1.0e-310, 2.0e-310, 2.2250738585072014e-308 }, { 5.0, 5.0, 5.0, 5.0, 5.0 }, { 0, 0, 0, 0, 0 }, kLimits, 0.0, 0.0, kNone);
	sequence("denormal-moving", { 0.0, 4.9e-324, 1.0e-310 }, { 5.0, 5.0, 5.0 }, { 0, 0, 0 }, kLimits, 2.0, 2.0, kNone);
	sequence("huge", { 1.0e15, 1.0e15 + 0.125, 1.0e15 + 0.25, 1.0e15 + 8.0 }, { 5.0, 5.0, 5.0, 5.0 }, { 0, 0, 1, 0 }, kLimits, 1.0, 0.0, kNone);
	sequence("huge-1e300", { 1.0e300, 1.0e300, 1.5e300 }, { 5.0, 2.0, 5.0 }, { 0, 0, 0 }, kLimits, 5.0, 5.0, kNone);
	// ---- steps
	step(0.0, 0.0, 0.0, 1.5, 2.5);
	step(0.0, 3.0, 2.0, 1.5, 2.5);
	step(0.1, 0.0, 0.0, 1.5, 2.5);
	step(0.1, 0.0, 1.0, 1.5, 2.5);
	step(0.1, 2.0, 0.0, 1.5, 2.5);
	step(4.9e-324, 0.0, 0.0, 1.5, 2.5);
	step(4.9e-324, 1.0, 1.0, 1.5, 2.5);
	step(1.0e300, 0.0, 0.0, 1.5, 2.5);
	step(1.0e300, 5.0, 5.0, 1.5, 2.5);
	for (int r = 0; r < 40; r++)
		step(uniform(0.0, 0.5), r % 4 ? uniform(0.0, 5.0) : 0.0, r % 5 ? uniform(0.0, 5.0) : 0.0, uniform(0.3, 3.0), uniform(0.3, 4.0));
	if (ppv::step_time(0.0, 0.0, 0.0, 1.5, 2.5) != 0.0 || ppv::step_time(0.0, 3.0, 2.0, 1.5, 2.5) != 0.0)
		fail("ds == 0 takes no time", "step", 0, 0.0, 0.0);
	// ---- directions, cusps, caps
	for (int own = -1; own <= 1; own++)
		for (int previous = -1; previous <= 1; previous++) {
			std::printf("D %d %d %d\n", own, previous, ppv::carried_direction(own, previous));
			std::printf("U %d %d %d\n", own, previous, (int)ppv::is_cusp(own, previous));
		}
	for (int r = 0; r < 60; r++) {
		ppv::Limits L = kLimits;
		L.clearanceGain = r % 3 ? uniform(0.1, 4.0) : 0.0;
		L.vFloor = r % 2 ? uniform(0.0, 1.0) : 0.0;
		const int direction = (int)(next() % 3) - 1;
		const double kappa = r % 4 ? uniform(0.0, 0.6) : 0.0;
		const float clearance = (float)uniform(0.0, 3.0);
		std::printf("K %d %a %a %a %a %a\n", direction, kappa, (double)clearance, L.clearanceGain, L.vFloor, ppv::cap(L, direction, kappa, clearance));
	}
	if (!ppv::lower_clearance(1.0, 5.0, 2.0, 0.0) || ppv::lower_clearance(2.0, 0.0, 1.0, 5.0) || !ppv::lower_clearance(1.0, 2.0, 1.0, 5.0) || ppv::lower_clearance(1.0, 5.0, 1.0, 5.0) ||
		!ppv::lower_clearance(1.0, 0.0, HUGE_VAL, 0.0))
		fail("the clearance minimum's tie rule", "clearance", 0, 0.0, 0.0);
	std::printf("speed rule ok\n");
	return 0;
}
