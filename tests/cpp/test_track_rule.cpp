// The rule of tracked movers in a delay call (pathplanning_amd/csrc/pp_track_rule.hpp) run on the host: the same text k_track_samples,
// k_delay_level_tracks and k_track_pairs compile for the device and the host side of the call runs.  A stand-alone program, built with
// -fsanitize=address,undefined and without contraction by tests/test_track_rule_host.py.  It checks itself (exit status 1 and a line on stderr at
// the first failure) and prints every value -- doubles as their 64 bits in hexadecimal -- which the Python test compares with tests/track_restatement.py.
//   T <name> <W>                                         a track follows
//   W <t> <x> <y>                                        one line per waypoint row
//   Q <what> <tau> <present: 0 / 1> <waypoint_of()> <x> <y>   one query of the track above (absent: waypoint -1, x = y = 0)
//   K <m> <n> <M> <partner> <key()> <time_of()> <partner_of()> <is_track()> <track_of_partner()>
//   V <name> <fault> <index> <track>                     one validation
// Checked here: a track is present exactly on [t_0, t_{W-1}], one ulp outside either end it is absent; on a waypoint time it is at the waypoint
// (lam == 0); the waypoint found brackets tau; just below the next waypoint's time lam < 1 and the position lies between the two rows; a key gives
// its time and partner back for M == 0 (the delay call's key) and M > 0, and every track's key at a time is above every vehicle's there; every
// refusal of validate() names its first offender, and nothing behind a fault is read (the arrays end at the fault: the sanitizer sees a read past
// them).
#include "pp_track_rule.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

namespace {

[[noreturn]] void fail(const char* what, double a, double b)
{
	std::fprintf(stderr, "FAILED %s: %.17g against %.17g\n", what, a, b);
	std::exit(1);
}

unsigned long long bits(double x)
{
	uint64_t u;
	std::memcpy(&u, &x, 8);
	return (unsigned long long)u;
}

uint64_t state = 0x9E3779B97F4A7C15ull;
double uniform() // [0, 1), from the high bits of a 64-bit LCG
{
	state = state * 6364136223846793005ull + 1442695040888963407ull;
	return (double)(state >> 11) * (1.0 / 9007199254740992.0);
}

void query(const char* what, const std::vector<double>& w, int W, double tau)
{
	double x = 0.0, y = 0.0;
	const bool present = ppk::position(w.data(), W, tau, x, y);
	const double t0 = w[0], tEnd = w[3 * (size_t)(W - 1)];
	if (present != (tau >= t0 && tau <= tEnd))
		fail("present exactly on [t_0, t_{W-1}]", tau, present);
	int j = -1;
	if (present) {
		j = ppk::waypoint_of(w.data(), W, tau);
		if (j < 0 || j >= W || !(w[3 * (size_t)j] <= tau) || (j + 1 < W && !(tau < w[3 * (size_t)(j + 1)])))
			fail("the waypoint found brackets tau", tau, j);
		if (tau == w[3 * (size_t)j] && (x != w[3 * (size_t)j + 1] || y != w[3 * (size_t)j + 2]))
			fail("on a waypoint time the track is at the waypoint", x, w[3 * (size_t)j + 1]);
		if (j + 1 < W) {
			const double xa = w[3 * (size_t)j + 1], xb = w[3 * (size_t)j + 4];
			if (x < std::fmin(xa, xb) - 1e-9 || x > std::fmax(xa, xb) + 1e-9) // (to rounding: lam <= 1, and one product and one sum are rounded)
				fail("the position lies between the two rows", x, xa);
		}
	} else
		x = y = 0.0;
	std::printf("Q %s %llx %d %d %llx %llx\n", what, bits(tau), present ? 1 : 0, j, bits(x), bits(y));
}

void track(const char* name, int W)
{
	std::vector<double> w(3 * (size_t)W); // (sized to the element: a read past the last row is seen)
	double t = -1.25 + uniform();
	for (int j = 0; j < W; j++) {
		w[3 * (size_t)j] = t;
		w[3 * (size_t)j + 1] = 40.0 * uniform() - 20.0;
		w[3 * (size_t)j + 2] = 40.0 * uniform() - 20.0;
		t += 0.01 + 0.7 * uniform();
	}
	std::printf("T %s %d\n", name, W);
	for (int j = 0; j < W; j++)
		std::printf("W %llx %llx %llx\n", bits(w[3 * (size_t)j]), bits(w[3 * (size_t)j + 1]), bits(w[3 * (size_t)j + 2]));
	const double inf = std::numeric_limits<double>::infinity();
	const double t0 = w[0], tEnd = w[3 * (size_t)(W - 1)];
	query("first", w, W, t0);
	query("last", w, W, tEnd);
	query("ulp-before", w, W, std::nextafter(t0, -inf));
	query("ulp-behind", w, W, std::nextafter(tEnd, inf));
	query("far-before", w, W, t0 - 1e6);
	query("far-behind", w, W, tEnd + 1e6);
	for (int j = 0; j < W; j++) {
		query("on", w, W, w[3 * (size_t)j]); // lam == 0
		if (j + 1 < W) {
			const double next = w[3 * (size_t)(j + 1)];
			const double below = std::nextafter(next, -inf); // lam just below 1
			const double lam = (below - w[3 * (size_t)j]) / (next - w[3 * (size_t)j]);
			if (!(lam <= 1.0))
				fail("lam does not exceed 1", lam, 1.0);
			query("below-next", w, W, below);
			query("above", w, W, std::nextafter(w[3 * (size_t)j], inf));
			query("mid", w, W, 0.5 * (w[3 * (size_t)j] + next));
		}
	}
	for (int q = 0; q < 40; q++)
		query("any", w, W, t0 - 0.5 + (tEnd - t0 + 1.0) * uniform());
}

void keys()
{
	const int64_t ns[] = { 1, 2, 48, 4096 };
	const int64_t Ms[] = { 0, 1, 3, 17, 1 << 16 };
	const int64_t ms[] = { 0, 1, 63, 64, (1 << 20) - 1 };
	for (int64_t n : ns)
		for (int64_t M : Ms)
			for (int64_t m : ms) {
				const int64_t partners[] = { 0, n - 1, M ? ppk::partner_of_track(n, 0) : 0, M ? ppk::partner_of_track(n, M / 2) : n - 1, M ? ppk::partner_of_track(n, M - 1) : n - 1 };
				for (int64_t p : partners) {
					const uint64_t k = ppk::key(m, n, M, p);
					if (ppk::time_of(k, n, M) != m || ppk::partner_of(k, n, M) != p || k == ppy::kNoKey)
						fail("a key gives its time and partner back", (double)ppk::time_of(k, n, M), (double)m);
					if (M == 0 && (k != ppy::key(m, n, p) || ppk::is_track(n, p)))
						fail("without tracks the key is the delay call's", (double)k, (double)ppy::key(m, n, p));
					if (ppk::is_track(n, p) && (ppk::partner_of_track(n, ppk::track_of_partner(n, p)) != p || ppk::track_of_partner(n, p) < 0 || ppk::track_of_partner(n, p) >= M))
						fail("a track's partner index gives the track back", (double)ppk::track_of_partner(n, p), (double)p);
					if (M && !ppy::before(ppk::key(m, n, M, n - 1), ppk::key(m, n, M, ppk::partner_of_track(n, 0))))
						fail("a track's key is above every vehicle's at that time", (double)m, (double)n);
					if (M && !ppy::before(ppk::key(m, n, M, ppk::partner_of_track(n, M - 1)), ppk::key(m + 1, n, M, 0)))
						fail("a later time's key is above every track's", (double)m, (double)n);
					std::printf("K %lld %lld %lld %lld %llu %d %d %d %lld\n", (long long)m, (long long)n, (long long)M, (long long)p, (unsigned long long)k, ppk::time_of(k, n, M),
						ppk::partner_of(k, n, M), ppk::is_track(n, p) ? 1 : 0, (long long)(ppk::is_track(n, p) ? ppk::track_of_partner(n, p) : -1));
				}
			}
}

void verdict(const char* name, int32_t M, int32_t reserved, const int32_t* offsets, const double* waypoints, const double* radii, int64_t T,
	ppk::Fault fault, int64_t index, int64_t trackOf)
{
	const ppk::Verdict v = ppk::validate(M, reserved, offsets, waypoints, radii, T);
	if (v.fault != fault || v.index != index || v.track != trackOf)
		fail(name, (double)v.fault * 1e9 + (double)v.index, (double)fault * 1e9 + (double)index);
	std::printf("V %s %d %lld %lld\n", name, (int)v.fault, (long long)v.index, (long long)v.track);
}

void validations()
{
	const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
	// three tracks of 2, 1 and 3 rows
	const std::vector<int32_t> offsets { 0, 2, 3, 6 };
	const std::vector<double> waypoints { 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, /**/ 5.0, 0.0, 0.0, /**/ -1.0, 3.0, 3.0, 0.0, 3.0, 4.0, 0.5, -3.0, 4.0 };
	const std::vector<double> radii { 0.0, 0.3, 1.0 };
	const std::vector<int32_t> noInts(1);
	const std::vector<double> noDoubles(1);
	const int32_t* const none = noInts.data() + 1; // not null, and not to be read: one behind the end of an array
	const double* const nothing = noDoubles.data() + 1;
	verdict("valid", 3, 0, offsets.data(), waypoints.data(), radii.data(), 601, ppk::kValid, -1, -1);
	verdict("no-tracks", 0, 0, nullptr, nullptr, nullptr, 601, ppk::kValid, -1, -1);
	verdict("no-tracks-empty-arrays", 0, 0, none, nothing, nothing, 1 << 20, ppk::kValid, -1, -1);
	{
		std::vector<int32_t> o(65);
		std::vector<double> w(3 * 64, 0.0), r(64, 0.5);
		for (int k = 0; k <= 64; k++)
			o[(size_t)k] = k;
		verdict("most-samples", 64, 0, o.data(), w.data(), r.data(), 1 << 20, ppk::kValid, -1, -1); // (64 * 2^20 == 2^26 samples are allowed)
		verdict("one-sample-more", 64, 0, o.data(), w.data(), r.data(), (1 << 20) + 1, ppk::kSampleCount, -1, -1);
	}
	verdict("reserved", 3, 1, offsets.data(), waypoints.data(), radii.data(), 601, ppk::kReserved, -1, -1);
	verdict("reserved-before-count", -1, 7, nullptr, nullptr, nullptr, 601, ppk::kReserved, -1, -1);
	verdict("negative-count", -1, 0, offsets.data(), waypoints.data(), radii.data(), 601, ppk::kCount, -1, -1);
	verdict("too-many-tracks", (1 << 16) + 1, 0, offsets.data(), waypoints.data(), radii.data(), 1, ppk::kCount, -1, -1);
	verdict("null-offsets", 3, 0, nullptr, waypoints.data(), radii.data(), 601, ppk::kNullOffsets, -1, -1);
	verdict("null-waypoints", 3, 0, offsets.data(), nullptr, radii.data(), 601, ppk::kNullWaypoints, -1, -1);
	verdict("null-radii", 3, 0, offsets.data(), waypoints.data(), nullptr, 601, ppk::kNullRadii, -1, -1);
	{
		const std::vector<int32_t> o { 1 }; // (nothing behind offsets[0] is read)
		verdict("first-offset", 3, 0, o.data(), nothing, nothing, 601, ppk::kFirstOffset, 0, -1);
	}
	{
		const std::vector<int32_t> o { 0, 2, 2 }; // track 1 owns no row
		verdict("empty-track", 3, 0, o.data(), nothing, nothing, 601, ppk::kOffsetOrder, 1, -1);
		const std::vector<int32_t> d { 0, 2, 3, 1 };
		verdict("offsets-descend", 3, 0, d.data(), nothing, nothing, 601, ppk::kOffsetOrder, 2, -1);
		const std::vector<int32_t> e { 0, 0 };
		verdict("empty-first-track", 1, 0, e.data(), nothing, nothing, 601, ppk::kOffsetOrder, 0, -1);
	}
	{
		const std::vector<int32_t> o { 0, (1 << 24) + 1 };
		verdict("too-many-waypoints", 1, 0, o.data(), nothing, nothing, 601, ppk::kWaypointCount, -1, -1);
	}
	verdict("too-many-samples", 3, 0, offsets.data(), nothing, nothing, (1 << 26) / 3 + 1, ppk::kSampleCount, -1, -1);
	for (int c = 0; c < 3; c++)
		for (double bad : { nan, inf, -inf }) {
			std::vector<double> w(waypoints.begin(), waypoints.begin() + 3 * 4); // rows 0 .. 3: the fault is in row 3, the first of track 2
			w[3 * 3 + (size_t)c] = bad;
			verdict(c == 0 ? "waypoint-time-not-finite" : (c == 1 ? "waypoint-x-not-finite" : "waypoint-y-not-finite"), 3, 0, offsets.data(), w.data(), nothing, 601, ppk::kWaypointValue, 3, 2);
		}
	{
		std::vector<double> w(waypoints.begin(), waypoints.begin() + 3 * 2);
		w[3] = w[0]; // equal times in track 0
		verdict("waypoint-times-equal", 3, 0, offsets.data(), w.data(), nothing, 601, ppk::kWaypointOrder, 1, 0);
		std::vector<double> v(waypoints.begin(), waypoints.begin() + 3 * 6);
		v[3 * 5] = -0.5; // the last row of track 2 goes back in time
		verdict("waypoint-times-descend", 3, 0, offsets.data(), v.data(), nothing, 601, ppk::kWaypointOrder, 5, 2);
		// (a track may begin before the one in front of it ends: the order holds within a track only -- `valid` above has track 2 begin at -1)
	}
	for (double bad : { -0.01, nan, inf, -inf }) {
		std::vector<double> r { 0.0, bad }; // (radii behind the fault are not read)
		verdict("radius", 3, 0, offsets.data(), waypoints.data(), r.data(), 601, ppk::kRadius, 1, -1);
	}
}

} // namespace

int main()
{
	track("one", 1);
	track("two", 2);
	track("sixty-four", 64);
	track("sixty-five", 65);
	track("hundred-thirty", 130);
	keys();
	validations();
	std::printf("track rule ok\n");
	return 0;
}
