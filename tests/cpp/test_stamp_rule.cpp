// The stamp's sample schedule and cell rule (pathplanning_amd/csrc/pp_stamp_rule.hpp) run on the host: the same text k_stamp_tickets compiles
// for the device.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_stamp_rule_host.py, which restates the rule
// in numpy and compares what this program prints, exactly (hex floats: every double crosses the pipe bit for bit).
//   S <L> <spacing> <n> <ratio 0> ... <ratio n>
//   C <rows> <cols> <res> <gx> <gy> <cx> <cy> <R> <row lo> <row hi> <col lo> <col hi> <covers() of every cell of the range, row-major, as 0/1>
#include "pp_stamp_rule.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
uint64_t next()
{ // splitmix64
	uint64_t z = (state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(next() >> 11) * (1.0 / 9007199254740992.0); }

void schedule(double L, double spacing)
{
	const int n = pps::edge_steps(L, spacing);
	std::printf("S %a %a %d", L, spacing, n);
	const int shown = n < 4096 ? n : 4096; // (the capped case prints its first ratios only)
	for (int k = 0; k <= shown; k++)
		std::printf(" %a", pps::sample_ratio(k, n));
	std::printf("\n");
}

void cells(const pps::Grid& g, double cx, double cy, double R)
{
	int r0, r1, c0, c1;
	pps::axis_range(cx, R, g.gx, g.res, g.rows, r0, r1);
	pps::axis_range(cy, R, g.gy, g.res, g.cols, c0, c1);
	std::printf("C %d %d %a %a %a %a %a %a %d %d %d %d ", g.rows, g.cols, g.res, g.gx, g.gy, cx, cy, R, r0, r1, c0, c1);
	if (r0 <= r1 && c0 <= c1)
		for (int r = r0; r <= r1; r++)
			for (int c = c0; c <= c1; c++)
				std::putchar(pps::covers(g, r, c, cx, cy, R) ? '1' : '0');
	else
		std::putchar('-');
	std::printf("\n");
}

} // namespace

int main()
{
	// ---- the schedule: L == 0, L < spacing, L an exact multiple of spacing, one step more than a multiple, random pairs, lengths that are no lengths
	schedule(0.0, 0.1);
	schedule(-0.0, 0.1);
	schedule(-1.0, 0.1);
	schedule(std::nan(""), 0.1);
	schedule(1e-300, 0.1);
	schedule(0.05, 0.1);
	schedule(0.1, 0.1);
	schedule(5.0, 1e-9); // capped
	for (int k = 1; k <= 24; k++) {
		schedule(0.25 * k, 0.25);                          // exact multiples (binary fractions: the quotient is the integer)
		schedule(0.25 * k + 1e-12, 0.25);                  // just beyond: one more, shorter step
		schedule(0.1 * k, 0.1);                            // decimal "multiples": whatever the double quotient says
		schedule((double)0.1f * k, (double)0.1f);
	}
	for (int i = 0; i < 60; i++)
		schedule(uniform(0.0, 6.0), i % 3 == 0 ? 0.37 : uniform(0.02, 1.5));
	// ---- the cell rule on grids with non-zero origins
	const pps::Grid grids[3] = { { 40, 50, (double)0.1f, -1.7, 2.3 }, { 23, 17, (double)0.15f, 100.05, -40.0 }, { 64, 64, 0.25, -8.0, -8.0 } };
	for (const pps::Grid& g : grids) {
		const double w = g.rows * g.res, h = g.cols * g.res;
		cells(g, g.gx + 0.5 * w, g.gy + 0.5 * h, 1.0);                        // inside
		cells(g, g.gx + 3.5 * g.res, g.gy + 7.5 * g.res, 0.0);                // R = 0 on a cell centre
		cells(g, g.gx + 3.5 * g.res, g.gy + 7.5 * g.res, 0.03);               // R below half a cell, on a centre: that cell
		cells(g, g.gx + 4.0 * g.res, g.gy + 8.0 * g.res, 0.03);               // ... on a corner: none
		cells(g, g.gx - 0.4, g.gy + 0.5 * h, 1.0);                            // partly outside, every side
		cells(g, g.gx + w + 0.4, g.gy + 0.5 * h, 1.0);
		cells(g, g.gx + 0.5 * w, g.gy - 0.4, 1.0);
		cells(g, g.gx + 0.5 * w, g.gy + h + 0.4, 1.0);
		cells(g, g.gx - 0.3, g.gy - 0.3, 1.0);                                // a corner
		cells(g, g.gx - 5.0, g.gy + 0.5 * h, 1.0);                            // wholly outside
		cells(g, g.gx + 0.5 * w, g.gy + h + 1.0 + 2.0 * g.res, 1.0);
		cells(g, g.gx - 1.0 - 0.5 * g.res, g.gy + 0.5 * h, 1.0);              // the box reaches in, the disc may not
		cells(g, 1e300, g.gy, 1.0);
		cells(g, -1e300, -1e300, 1.0);
		cells(g, HUGE_VAL, g.gy, 1.0);
		cells(g, g.gx, -HUGE_VAL, 1.0);
		cells(g, std::nan(""), g.gy, 1.0);
		cells(g, g.gx + 0.5 * w, g.gy + 0.5 * h, 100.0);                      // the whole grid
		for (int i = 0; i < 70; i++)
			cells(g, uniform(g.gx - 1.5, g.gx + w + 1.5), uniform(g.gy - 1.5, g.gy + h + 1.5), i % 5 == 0 ? uniform(0.0, 0.08) : uniform(0.1, 1.6));
	}
	// ---- the small pieces
	std::printf("W %d %d %d %d\n", pps::in_window(1.0, 1.0, 1.0), pps::in_window(1.0, 1.5, 0.5), pps::in_window(0.0, -HUGE_VAL, HUGE_VAL), pps::in_window(2.0, 0.0, 1.0));
	std::printf("R %a %a\n", pps::effective_radius(1.0f, 0.12f), pps::sample_arc_length(3.0, 0.5, 0.7));
	return 0;
}
