// The rule of a call with waits at stops (pathplanning_amd/csrc/pp_wait_rule.hpp) run on the host: the same text k_wait_places and k_wait_level
// compile for the device.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_wait_rule_host.py.  It checks itself (exit
// status 1 and a line on stderr at the first failure) and prints every value, which the Python test compares with tests/wait_restatement.py.
//   S <T> <D> <a> <d> <c> <source()>             the position under a wait at a stop, for every c (-1: standing)
//   W <D> <d> <c> <source_start()>               ... at the start
//   A <kE> <columns> <dt> <tStart> <tArrive> <arrive_column()>    doubles as C99 hexadecimal floats
//   F <row> <N> <a> <D> <columns> <is_place()> <fixed_qualifies() of a standing row>
//   O <D> <S> <P> <ordinal> <place> <d>          candidate() of every ordinal, in order
//   N <D> <S> <P> <candidates()>
//   X <T> <D> <a> <d> <m0> <rejected_with_the_first()> <m of the exhaustive evaluation, -1: clear>
// Checked here: a source is a column inside 0 .. T + D - 1 or standing, standing exactly for a <= c < a + d; the arc length of a monotone trajectory
// read through source() never decreases in c when the stop lies between columns a - 1 and a; the arrive column is the first column at or behind
// t_arrive (the one before it is before it) for t_arrive itself and one ulp either side; ordinal() and candidate() invert each other and follow a
// plain loop; on random small instances a candidate the shortcut rejects is rejected by the exhaustive evaluation at the same time.
#include "pp_wait_rule.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

[[noreturn]] void fail(const char* what, long long a, long long b)
{
	std::fprintf(stderr, "FAILED %s: %lld against %lld\n", what, a, b);
	std::exit(1);
}

void sources(int T, int D)
{
	const int64_t columns = (int64_t)T + D;
	const int64_t as[] = { 0, D, columns - 1, columns };
	const int64_t ds[] = { 0, 1, D };
	for (int64_t a : as)
		for (int64_t d : ds) {
			if (d > D)
				continue;
			long long before = -(1ll << 40);
			for (int64_t c = D; c < columns; c++) { // (c = m + D for m = 0 .. T - 1)
				const int64_t at = ppw::source(c, a, d);
				const bool standing = d > 0 && a <= c && c < a + d;
				if ((at == ppw::kStanding) != standing)
					fail("standing exactly inside the wait", at, c);
				if (!standing && (at < 0 || at >= columns || at != (c < a || d == 0 ? c : c - d)))
					fail("a source is a column of the extended trajectory", at, c);
				// twice the arc length of a trajectory with s(column) = column, the stop between columns a - 1 and a
				const long long s2 = standing ? 2 * a - 1 : 2 * at;
				if (s2 < before)
					fail("the arc length never decreases", s2, before);
				before = s2;
				std::printf("S %d %d %lld %lld %lld %lld\n", T, D, (long long)a, (long long)d, (long long)c, (long long)at);
			}
		}
	for (int64_t d : ds) {
		if (d > D)
			continue;
		for (int64_t c = D; c < columns; c++) {
			const int64_t at = ppw::source_start(c, d);
			if (at < 0 || at >= columns)
				fail("a start wait reads a column of the extended trajectory", at, c);
			std::printf("W %d %lld %lld %lld\n", D, (long long)d, (long long)c, (long long)at);
		}
	}
}

void arrivals()
{
	struct Case {
		int64_t kE, columns;
		double dt, tStart;
	};
	const Case cases[] = { { 7, 130, 0.1, 0.0123 }, { -58, 195, 0.1, -2.7317 }, { 0, 1, 0.5, 0.0 }, { -3000, 901, 0.05, 1e-3 }, { 1ll << 40, 64, 0.1, 109951162777.6 } };
	for (const Case& k : cases) {
		std::vector<double> wanted { -1.0, 0.0, 1e300 };
		for (int64_t c : { (int64_t)0, k.columns / 2, k.columns - 1 })
			wanted.push_back(ppw::since_start(k.kE, c, k.dt, k.tStart)); // (exactly a column's time)
		wanted.push_back(0.37);
		wanted.push_back(3.0 * k.dt + 0.01);
		for (double t : wanted)
			for (int side = -1; side <= 1; side++) {
				const double tArrive = side < 0 ? std::nextafter(t, -INFINITY) : (side > 0 ? std::nextafter(t, INFINITY) : t);
				const int64_t a = ppw::arrive_column(k.kE, k.columns, k.dt, k.tStart, tArrive);
				if (a < 0 || a > k.columns)
					fail("the arrive column lies in 0 .. columns", a, k.columns);
				if (a < k.columns && !(ppw::since_start(k.kE, a, k.dt, k.tStart) >= tArrive))
					fail("the arrive column is at or behind the arrival", a, 0);
				if (a > 0 && ppw::since_start(k.kE, a - 1, k.dt, k.tStart) >= tArrive)
					fail("the column before the arrive column is before the arrival", a, 0);
				std::printf("A %lld %lld %a %a %a %lld\n", (long long)k.kE, (long long)k.columns, k.dt, k.tStart, tArrive, (long long)a);
			}
	}
}

void filters()
{
	const int64_t N = 9, D = 4, columns = 12;
	for (int64_t row : { (int64_t)-1, (int64_t)0, (int64_t)1, N - 2, N - 1, N })
		for (int64_t a : { (int64_t)0, D - 1, D, columns - 1, columns })
			std::printf("F %lld %lld %lld %lld %lld %d %d\n", (long long)row, (long long)N, (long long)a, (long long)D, (long long)columns, ppw::is_place(row, N, a, D, columns) ? 1 : 0,
				ppw::fixed_qualifies(row, N, true, a, columns) ? 1 : 0);
	if (ppw::fixed_qualifies(3, N, false, 0, columns))
		fail("a row that moves is no stop", 1, 0);
}

void orders()
{
	for (int64_t D : { (int64_t)0, (int64_t)1, (int64_t)5 })
		for (int64_t S : { (int64_t)0, (int64_t)1 })
			for (int64_t P : { (int64_t)0, (int64_t)1, (int64_t)4 }) {
				const int64_t n = ppw::candidates(D, S, P);
				std::printf("N %lld %lld %lld %lld\n", (long long)D, (long long)S, (long long)P, (long long)n);
				int64_t o = 0; // the plain loop
				int place, d;
				ppw::candidate(o, S, P, place, d);
				if (place != ppw::kNoWait || d != 0)
					fail("candidate 0 is no wait", place, d);
				std::printf("O %lld %lld %lld %lld %d %d\n", (long long)D, (long long)S, (long long)P, (long long)o, place, d);
				o++;
				for (int64_t dd = 1; dd <= D; dd++)
					for (int64_t q = -S; q < P; q++, o++) {
						ppw::candidate(o, S, P, place, d);
						if (place != (q < 0 ? ppw::kStart : (int)q) || d != dd)
							fail("candidate() follows the plain loop", place, q);
						if (ppw::ordinal(place, d, S, P) != o)
							fail("ordinal() inverts candidate()", ppw::ordinal(place, d, S, P), o);
						std::printf("O %lld %lld %lld %lld %d %d\n", (long long)D, (long long)S, (long long)P, (long long)o, place, d);
					}
				if (o != n)
					fail("candidates() counts the plain loop", o, n);
			}
}

/// the least time in 0 .. T - 1 at which a vehicle at p[source] (standing: at `stop`) meets a partner at q[m]; -1: never
int64_t first_meeting(const std::vector<int>& p, const std::vector<int>& q, int T, int D, int64_t a, int64_t d, int stop)
{
	for (int m = 0; m < T; m++) {
		const int64_t at = ppw::source(m + D, a, d);
		if ((at == ppw::kStanding ? stop : p[(size_t)at]) == q[(size_t)m])
			return m;
	}
	return -1;
}

void shortcut()
{
	uint64_t lcg = 77;
	auto draw = [&](int n) {
		lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
		return (int)((lcg >> 33) % (uint64_t)n);
	};
	int taken = 0;
	for (int round = 0; round < 400; round++) {
		const int T = 1 + draw(12), D = draw(6), columns = T + D;
		std::vector<int> p((size_t)columns), q((size_t)T);
		int s = draw(3);
		for (int& x : p)
			x = (s += draw(2));
		for (int& x : q)
			x = draw(s + 2);
		const int64_t m0 = first_meeting(p, q, T, D, 0, 0, 0);
		for (int64_t a = D; a <= columns; a++)
			for (int64_t d = 1; d <= D; d++) {
				const int stop = a < columns ? p[(size_t)a] : s;
				const bool skip = m0 >= 0 && ppw::rejected_with_the_first(a, m0, D);
				const int64_t m = first_meeting(p, q, T, D, a, d, stop);
				if (skip && m != m0)
					fail("a candidate the shortcut rejects is rejected at the same time", m, m0);
				taken += skip;
				std::printf("X %d %d %lld %lld %lld %d %lld\n", T, D, (long long)a, (long long)d, (long long)m0, skip ? 1 : 0, (long long)m);
			}
	}
	if (taken < 100)
		fail("the shortcut is taken on the random instances", taken, 100);
}

} // namespace

int main()
{
	sources(1, 0);
	sources(1, 3);
	sources(5, 3);
	sources(64, 65);
	arrivals();
	filters();
	orders();
	shortcut();
	std::printf("wait rule ok\n");
	return 0;
}
