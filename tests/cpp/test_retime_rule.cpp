// The rule of a retime call (pathplanning_amd/csrc/pp_retime_rule.hpp) run on the host: the same text k_retime_tickets compiles for the device.  A
// stand-alone program, built without contraction with -fsanitize=address,undefined by tests/test_retime_rule_host.py.  It checks itself (exit status 1
// and a line on stderr at the first failure) and prints every value, doubles as C99 hexadecimal floats, which the Python test compares with
// tests/retime_restatement.py bit for bit.
//   Q <name> <N> <a_acc> <a_dec>        a profile; then its rows:  R <s> <v> <t>
//   D <r> <dwell()>                     every row r >= 1
//   C <case> <count>                    a list of holds for the profile; then  G <row> <seconds> <hold_status() on the original rows> <P_h>
//   K <k> <hold_of()>                   every row k
//   T <k> <t'_k>                        every row after the rewrite (only for a list without an offender)
// Checked here: the prefix is the sequential sum in list order (1e16, 1, -1e16 gives 0, not 1); hold_of at a hold's row is that hold, one row before it
// the hold before (-1 before the first), behind the last hold the last; a hold of exactly minus the dwell is valid and one ulp below it is not; a hold on
// a moving row is no stop, whatever its seconds; a hold at N - 1 moves that row alone; after the rewrite the times never decrease inside one hold
// segment, rows before the first hold keep their bits, and s and v keep theirs everywhere.
#include "pp_retime_rule.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

[[noreturn]] void fail(const char* what, const std::string& where, double a, double b)
{
	std::fprintf(stderr, "FAILED %s (%s): %a against %a\n", what, where.c_str(), a, b);
	std::exit(1);
}

struct Hold { // pp_hold's layout
	int32_t plan, row;
	double seconds;
};
static_assert(sizeof(Hold) == 16 && sizeof(Hold) == ppr::kHoldInts * 4 && sizeof(Hold) == ppr::kHoldDoubles * 8, "pp_hold layout");

struct Profile {
	std::string name;
	double aAcc, aDec;
	std::vector<double> rows; // (s, v, t)
	int N() const { return (int)(rows.size() / 3); }
};

/// rows from arc lengths, speeds and the dwell of every row, as the speed profile forms the times: t_j = t_{j-1} + (step_time + dwell_j)
Profile make(const std::string& name, const std::vector<double>& s, const std::vector<double>& v, const std::vector<double>& dwell, double aAcc = 1.5, double aDec = 2.5)
{
	Profile p { name, aAcc, aDec, {} };
	double t = 0.0;
	for (size_t j = 0; j < s.size(); j++) {
		if (j > 0)
			t = t + (ppv::step_time(s[j] - s[j - 1], v[j - 1], v[j], aAcc, aDec) + dwell[j]);
		p.rows.insert(p.rows.end(), { s[j], v[j], t });
	}
	return p;
}

uint64_t lcg(uint64_t& x) { return x = x * 6364136223846793005ull + 1442695040888963407ull; }
double unit(uint64_t& x) { return (double)(lcg(x) >> 11) / 9007199254740992.0; }

/// a profile of N rows that stands at row 0, at N - 1 and at every row whose index is a multiple of `every` (those dwell), and moves elsewhere
Profile stopping(const std::string& name, int N, int every, uint64_t seed)
{
	std::vector<double> s(N), v(N), dwell(N, 0.0);
	double at = 0.0;
	for (int j = 0; j < N; j++) {
		const bool stands = j == 0 || j == N - 1 || j % every == 0;
		if (j > 0)
			at += 0.05 + 0.3 * unit(seed);
		s[j] = at;
		v[j] = stands ? 0.0 : 0.2 + 2.0 * unit(seed);
		if (stands && j > 0 && j < N - 1)
			dwell[j] = 0.25 + unit(seed);
	}
	return make(name, s, v, dwell);
}

void print_profile(const Profile& p)
{
	std::printf("Q %s %d %a %a\n", p.name.c_str(), p.N(), p.aAcc, p.aDec);
	for (int j = 0; j < p.N(); j++)
		std::printf("R %a %a %a\n", p.rows[3 * j], p.rows[3 * j + 1], p.rows[3 * j + 2]);
	for (int r = 1; r < p.N(); r++) {
		const double d = ppr::dwell(p.rows.data(), r, p.aAcc, p.aDec);
		if (ppm::is_stop(p.rows[3 * r + 1]) && !(d >= -1e-12))
			fail("a stop's dwell is not negative beyond rounding", p.name, d, 0.0);
		std::printf("D %d %a\n", r, d);
	}
}

/// one list of holds on a profile: statuses on the original rows, the prefix, h(k), and -- without an offender -- the rewrite, checked and printed
void run_case(const Profile& p, const std::string& name, const std::vector<Hold>& holds, int wantStatus)
{
	const int N = p.N(), count = (int)holds.size();
	const std::string where = p.name + " / " + name;
	std::vector<double> P((size_t)count + 1, 0.0);
	const double held = count ? ppr::prefix(&holds[0].seconds, ppr::kHoldDoubles, count, P.data()) : ppr::prefix(nullptr, ppr::kHoldDoubles, 0, P.data());
	double plain = 0.0;
	for (int h = 0; h < count; h++) {
		plain = h == 0 ? holds[h].seconds : plain + holds[h].seconds;
		if (std::memcmp(&plain, &P[h], 8) != 0)
			fail("the prefix is the sequential sum", where, P[h], plain);
	}
	if (std::memcmp(&plain, &held, 8) != 0)
		fail("prefix() returns the last P", where, held, plain);
	std::printf("C %s %d\n", name.c_str(), count);
	int status = ppr::kApplied;
	for (int h = 0; h < count; h++) {
		const int st = ppr::hold_status(p.rows.data(), N, holds[h].row, holds[h].seconds, p.aAcc, p.aDec);
		if (status == ppr::kApplied)
			status = st;
		std::printf("G %d %a %d %a\n", holds[h].row, holds[h].seconds, st, P[h]);
	}
	if (status != wantStatus)
		fail("the status of the first offender", where, status, wantStatus);
	for (int k = 0; k < N; k++) {
		const int h = count ? ppr::hold_of(&holds[0].row, ppr::kHoldInts, count, k) : -1;
		int want = -1;
		for (int i = 0; i < count; i++)
			if (holds[i].row <= k)
				want = i;
		if (h != want)
			fail("hold_of is the last hold at or before the row", where, h, want);
		std::printf("K %d %d\n", k, h);
	}
	for (int h = 0; h < count; h++) { // at a hold's row, one row before it, behind the last
		if (ppr::hold_of(&holds[0].row, ppr::kHoldInts, count, holds[h].row) != h || ppr::hold_of(&holds[0].row, ppr::kHoldInts, count, holds[h].row - 1) != h - 1)
			fail("hold_of at a hold's row and before it", where, h, holds[h].row);
	}
	if (count && ppr::hold_of(&holds[0].row, ppr::kHoldInts, count, 1 << 30) != count - 1)
		fail("hold_of behind the last hold", where, count, 0);
	if (status != ppr::kApplied)
		return;
	std::vector<double> after = p.rows;
	for (int k = 0; k < N; k++) {
		const int h = count ? ppr::hold_of(&holds[0].row, ppr::kHoldInts, count, k) : -1;
		if (h >= 0)
			after[3 * k + 2] = ppr::retimed(p.rows[3 * k + 2], P[h]);
	}
	for (int k = 0; k < N; k++) {
		const int h = count ? ppr::hold_of(&holds[0].row, ppr::kHoldInts, count, k) : -1;
		if (std::memcmp(&after[3 * k], &p.rows[3 * k], 16) != 0)
			fail("s and v keep their bits", where, k, 0);
		if (h < 0 && std::memcmp(&after[3 * k + 2], &p.rows[3 * k + 2], 8) != 0)
			fail("rows before the first hold keep their bits", where, k, 0);
		if (k > 0 && h >= 0 && ppr::hold_of(&holds[0].row, ppr::kHoldInts, count, k - 1) == h && p.rows[3 * k + 2] >= p.rows[3 * (k - 1) + 2] &&
			!(after[3 * k + 2] >= after[3 * (k - 1) + 2]))
			fail("times never decrease inside one hold segment", where, after[3 * k + 2], after[3 * (k - 1) + 2]);
		std::printf("T %d %a\n", k, after[3 * k + 2]);
	}
}

} // namespace

int main()
{
	// the order of the prefix: sequential, in list order
	{
		const Hold big[3] = { { 0, 1, 1e16 }, { 0, 2, 1.0 }, { 0, 3, -1e16 } };
		double P[3];
		const double held = ppr::prefix(&big[0].seconds, ppr::kHoldDoubles, 3, P);
		if (P[0] != 1e16 || P[1] != 1e16 || P[2] != 0.0 || held != 0.0)
			fail("1e16 + 1 - 1e16 summed in list order is 0", "prefix", held, 0.0);
	}
	std::vector<Profile> profiles;
	profiles.push_back(make("junction-cusp-dwell", { 0.0, 0.5, 1.0, 1.5, 2.0, 2.0, 2.0, 2.6, 3.2, 3.2 }, { 0.0, 1.0, 1.5, 1.0, 0.5, 0.0, 0.0, 0.9, 0.0, 0.0 },
		{ 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.25, 0.0, 0.0, 0.5 }));
	profiles.push_back(make("two-standing", { 0.0, 2.0 }, { 0.0, 0.0 }, { 0.0, 0.0 }));
	profiles.push_back(stopping("short-40", 40, 7, 11));
	profiles.push_back(stopping("rows-63-64-65", 150, 1 << 20, 12)); // (its stops are put at 63, 64 and 65 below)
	{
		Profile& p = profiles.back();
		std::vector<double> s, v, dwell(150, 0.0);
		for (int j = 0; j < 150; j++) {
			s.push_back(p.rows[3 * j]);
			v.push_back(j == 63 || j == 64 || j == 65 || j == 128 ? 0.0 : p.rows[3 * j + 1]);
		}
		dwell[63] = 0.5;
		dwell[65] = 0.75;
		dwell[128] = 0.1;
		p = make("rows-63-64-65", s, v, dwell);
	}
	profiles.push_back(stopping("long-200", 200, 9, 13));
	for (const Profile& p : profiles) {
		print_profile(p);
		const int N = p.N();
		std::vector<int> stops, dwelt, moving;
		for (int r = 1; r < N; r++) {
			if (!ppm::is_stop(p.rows[3 * r + 1]))
				moving.push_back(r);
			else {
				stops.push_back(r);
				if (ppr::dwell(p.rows.data(), r, p.aAcc, p.aDec) > 0.1)
					dwelt.push_back(r);
			}
		}
		run_case(p, "none", {}, ppr::kApplied);
		run_case(p, "last-row", { { 0, N - 1, 2.5 } }, ppr::kApplied);
		{
			std::vector<Hold> every;
			uint64_t seed = 99 + (uint64_t)N;
			for (int r : stops)
				every.push_back({ 0, r, 0.1 + 3.0 * unit(seed) });
			run_case(p, "every-stop", every, ppr::kApplied);
			if (every.size() > 1) {
				std::vector<Hold> ends = { every.front(), every.back() };
				ends.back().seconds = 1e-9;
				run_case(p, "first-and-last-stop", ends, ppr::kApplied);
			}
		}
		if (!moving.empty()) {
			run_case(p, "moving-row", { { 0, moving[moving.size() / 2], 1.0 } }, ppr::kNotAStop);
			run_case(p, "moving-row-negative", { { 0, moving[0], -1e9 } }, ppr::kNotAStop); // (the stop test comes first)
		}
		for (int r : dwelt) { // delta + w == 0 exactly, and one ulp below
			const double delta = ppr::dwell(p.rows.data(), r, p.aAcc, p.aDec);
			run_case(p, "minus-the-dwell-" + std::to_string(r), { { 0, r, -delta } }, ppr::kApplied);
			run_case(p, "one-ulp-below-" + std::to_string(r), { { 0, r, std::nextafter(-delta, -INFINITY) } }, ppr::kNegativeDwell);
			if (r != stops.front())
				run_case(p, "offender-second-" + std::to_string(r), { { 0, stops.front(), 0.5 }, { 0, r, -delta - 1.0 } }, ppr::kNegativeDwell);
		}
		if (dwelt.empty() && p.name != "two-standing")
			fail("the profile has a dwelling stop", p.name, 0, 0);
	}
	std::printf("retime rule ok\n");
	return 0;
}
