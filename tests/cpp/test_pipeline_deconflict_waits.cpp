// HybridAStarPipeline::DeconflictWaits (pp_pipeline_deconflict_waits) through the C++ mirror: plans are held by ticket, profiled on the device
// (SpeedProfile) and given waits at their start or at their stops there, and every record is compared with a plain sequential loop made here over the
// device's own poses and places: Conflicts(..., withPoses) over the horizon that begins max_delay_steps lattice steps earlier returns the extended
// trajectory, the call returns every vehicle's places with their standing poses, and the loop below -- vehicles in index order, candidates in the
// header's order, EVERY one of them evaluated (the kernel takes the header's shortcut), times ascending, partners ascending -- is the rule of
// include/pp_hip.h written out.  The separation is the distance of the two poses minus twice the validator's min_safe_radius, in the header's order
// and without contraction, so every integer field and every time is compared EXACTLY.  With and without start waits, over every pair and over a
// chain, then the result fed back as fixed, and a ticket without a profile.  Needs a GPU.
#undef NDEBUG
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <map>
#include <thread>

#include "../../pathplanning_amd/host/map_authoring.hpp"

using namespace Planner;

namespace {

using Limits = HybridAStarPipeline::SpeedLimits;
using Horizon = HybridAStarPipeline::ConflictHorizon;
using Wait = HybridAStarPipeline::Wait;
using WaitPlace = HybridAStarPipeline::WaitPlace;
using FixedWait = HybridAStarPipeline::FixedWait;

Ref<Obstacle> wall(double dx, double dy, double x, double y, double theta)
{
	Ref<Obstacle> o = makeRef<Obstacle>();
	o->SetShape(makeRef<RectangleShape>(dx, dy));
	o->SetPose(Pose2d(x, y, theta));
	return o;
}

struct Expected {
	int status = -1, place = -2, row = -1, steps = -1, tried = 0, blocker = -1;
	double tStart = 0.0, tHold = 0.0, tResume = 0.0, sWait = 0.0, tBlock = 0.0;
};

struct Candidate {
	int place, d;
};

/// where vehicle i is at column c under (place, d): false where it is absent
bool at(const HybridAStarPipeline::Trajectory& plan, const std::vector<WaitPlace>& places, int place, int d, int c, double& x, double& y)
{
	int from = c;
	if (place == -1)
		from = c - d;
	else if (place >= 0 && d > 0 && c >= places[(size_t)place].column) {
		if (c < places[(size_t)place].column + d) {
			x = places[(size_t)place].pose.x();
			y = places[(size_t)place].pose.y();
			return true;
		}
		from = c - d;
	}
	const Pose2d& p = plan.poses[(size_t)from];
	x = p.x();
	y = p.y();
	return !std::isnan(x);
}

/// the rule, one vehicle after the other; poses[i] holds T + D columns, NaN where absent; below[i]: the partners of smaller index
std::vector<Expected> loop(const std::vector<HybridAStarPipeline::Trajectory>& plans, const std::vector<std::vector<WaitPlace>>& places, const std::vector<std::vector<int>>& below,
	const std::vector<double>& tStart, const std::vector<bool>& noStart, const std::vector<FixedWait>& fixed, const Horizon& h, long long k0, int T, int D, double R)
{
	const size_t n = plans.size();
	std::vector<Expected> out(n);
	for (size_t i = 0; i < n; i++) {
		Expected& e = out[i];
		if (plans[i].status == HybridAStarPipeline::Trajectory::Status::NoProfile)
			continue;
		const bool isFixed = !fixed.empty() && fixed[i].row != -2; // (a committed wait: its one candidate, scheduled whatever it meets; its list of places is its one row)
		std::vector<Candidate> tried { { -2, 0 } };
		if (isFixed)
			tried = { { fixed[i].steps == 0 ? -2 : (fixed[i].row == -1 ? -1 : 0), fixed[i].steps } };
		for (int d = 1; d <= D && !isFixed; d++) {
			if (noStart.empty() || !noStart[i])
				tried.push_back({ -1, d });
			for (int q = 0; q < (int)places[i].size(); q++)
				tried.push_back({ q, d });
		}
		for (const Candidate& cand : tried) {
			int mHit = -1, jHit = -1;
			for (int m = 0; m < T && mHit < 0; m++) {
				double ax, ay;
				if (!at(plans[i], places[i], cand.place, cand.d, m + D, ax, ay))
					continue;
				for (int j : below[i]) {
					const Expected& o = out[(size_t)j];
					if (o.steps < 0 || (jHit >= 0 && j >= jHit))
						continue;
					double bx, by;
					if (!at(plans[(size_t)j], places[(size_t)j], o.place, o.steps, m + D, bx, by))
						continue;
					const double dx = ax - bx, dy = ay - by;
					if (std::sqrt(dx * dx + dy * dy) - (R + R) < h.margin) {
						mHit = m;
						jHit = j;
					}
				}
			}
			e.tried++;
			if (mHit < 0 || isFixed) {
				e.status = mHit < 0 ? 0 : 2;
				e.steps = cand.d;
				e.place = cand.place;
			}
			if (mHit < 0)
				break;
			e.blocker = jHit;
			e.tBlock = (double)(k0 + mHit) * h.dt;
		}
		if (e.steps < 0)
			e.status = 1;
		e.tStart = e.steps >= 0 && e.place < 0 ? tStart[i] + (double)e.steps * h.dt : tStart[i];
		if (e.place >= 0) {
			const WaitPlace& pl = places[i][(size_t)e.place];
			e.row = pl.row;
			e.tHold = (double)(k0 - D + pl.column) * h.dt;
			e.tResume = (double)(k0 - D + pl.column + e.steps) * h.dt;
			e.sWait = pl.s;
		}
	}
	return out;
}

void compare(const std::vector<Wait>& got, const std::vector<Expected>& want, int& atStart, int& atStop)
{
	assert(got.size() == want.size());
	for (size_t i = 0; i < got.size(); i++) {
		const Wait& g = got[i];
		const Expected& w = want[i];
		if (!((int)g.status == w.status && g.place == w.place && g.row == w.row && g.waitSteps == w.steps && g.numTried == w.tried && g.blocker == w.blocker && g.tStart == w.tStart &&
				g.tHold == w.tHold && g.tResume == w.tResume && g.sWait == w.sWait && g.tBlock == w.tBlock)) {
			std::printf("vehicle %zu: (%d %d %d %d %d %d %.17g %.17g %.17g %.17g) on the device, (%d %d %d %d %d %d %.17g %.17g %.17g %.17g) by the loop\n", i, (int)g.status, g.place,
				g.row, g.waitSteps, g.numTried, g.blocker, g.tStart, g.tHold, g.tResume, g.tBlock, w.status, w.place, w.row, w.steps, w.tried, w.blocker, w.tStart, w.tHold, w.tResume,
				w.tBlock);
			assert(false);
		}
		assert(g.blocker >= 0 || (g.tBlock == 0.0 && g.sBlock[0] == 0.0 && g.sBlock[1] == 0.0));
		assert(g.sBlock[0] >= 0.0 && g.sBlock[1] >= 0.0 && (g.place >= 0 || g.sWait == 0.0));
		atStart += g.place == -1;
		atStop += g.place >= 0;
	}
}

} // namespace

int main()
{
	std::array<Pose2d, 2> bounds = { Pose2d(-10, -10, -M_PI), Pose2d(10, 10, M_PI) };
	Ref<StateSpaceSE2> space = makeRef<StateSpaceSE2>(bounds);
	const double walls[2][5] = { { 8.0, 0.6, -5.0, 1.0, 0.0 }, { 8.0, 0.6, 5.5, -2.0, 0.3 } };
	Ref<ObstacleListOccupancyMap> map = makeRef<ObstacleListOccupancyMap>(0.1f);
	Ref<StateValidatorOccupancyMap> validator = makeRef<StateValidatorOccupancyMap>(space, map);
	for (const auto& wl : walls)
		assert(map->AddObstacle(wall(wl[0], wl[1], wl[2], wl[3], wl[4])));
	GVD(map).Update();

	const int n = 12, maxNodes = 32768;
	HybridAStar::SearchParameters params;
	HybridAStarPipeline pipe(params, 16, maxNodes, 16);
	uint64_t lcg = 4242;
	auto uniform = [&](double lo, double hi) {
		lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
		return lo + (hi - lo) * (double)(lcg >> 11) / 9007199254740992.0;
	};
	auto validPose = [&]() {
		for (int tries = 0; tries < 100000; tries++) {
			const Pose2d p(uniform(-9.0, 9.0), uniform(-9.0, 9.0), uniform(-M_PI, M_PI));
			if (validator->IsStateValid(p))
				return p;
		}
		assert(!"no valid pose in 100000 draws");
		return Pose2d();
	};
	std::vector<Pose2d> starts, goals;
	std::vector<uint64_t> seeds;
	for (int i = 0; i < n; i++) {
		starts.push_back(validPose());
		goals.push_back(i == n - 1 ? starts.back() : validPose()); // the last query: start == goal, a one-pose plan
		seeds.push_back(9100 + (uint64_t)i);
	}
	assert(pipe.Initialize(validator));
	std::vector<uint64_t> tickets;
	assert(pipe.Submit(starts, goals, seeds, &tickets) == n);
	std::vector<uint64_t> held;
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<HybridAStarPipeline::Result> out;
	while ((int)held.size() < n) {
		pipe.Poll(out, 4096, true);
		for (const auto& r : out)
			held.push_back(r.ticket);
		if (out.empty())
			std::this_thread::sleep_for(std::chrono::microseconds(200));
		assert(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(60));
	}
	const double spacing = 0.2, R = 1.0; // (the validator's min_safe_radius)
	Limits L;
	L.dwell = 0.75;
	pipe.SpeedProfile(held, spacing, L);
	std::vector<double> tStart;
	for (size_t k = 0; k < held.size(); k++)
		tStart.push_back(0.3 + 0.11 * (double)k);
	std::vector<std::vector<int>> every(held.size()), chain(held.size());
	std::vector<std::pair<int, int>> chainPairs;
	for (int i = 0; i < (int)held.size(); i++) {
		for (int j = 0; j < i; j++)
			every[(size_t)i].push_back(j);
		if (i > 0) {
			chain[(size_t)i].push_back(i - 1);
			chainPairs.push_back(i % 2 ? std::make_pair(i, i - 1) : std::make_pair(i - 1, i));
		}
	}
	int atStart = 0, atStop = 0, atFixedStop = 0, calls = 0, fedBack = 0;
	const int maxPlaces = 3;
	for (int variant = 0; variant < 3; variant++) {
		Horizon h;
		h.tFrom = 0.0;
		h.tTo = 14.05;
		h.dt = 0.1;
		h.margin = 1.0;
		h.holdBefore = variant == 1;
		h.holdAfter = variant >= 1;
		for (int D : { 0, 40 }) {
			const long long k0 = (long long)std::ceil(h.tFrom / h.dt), k1 = (long long)std::floor(h.tTo / h.dt);
			const int T = (int)(k1 - k0 + 1);
			Horizon extended = h; // the lattice indices k0 - D .. k1: half a step before the first one
			extended.tFrom = ((double)(k0 - D) - 0.5) * h.dt;
			const HybridAStarPipeline::Conflicted traj = pipe.Conflicts(held, tStart, extended, true);
			assert(traj.plans.size() == held.size() && (int)traj.plans[0].poses.size() == T + D);
			for (int barred = 0; barred < 2; barred++) {
				const std::vector<bool> noStart = barred ? std::vector<bool>(held.size(), true) : std::vector<bool>();
				std::vector<std::vector<WaitPlace>> places;
				const std::vector<Wait> all = pipe.DeconflictWaits(held, tStart, {}, true, h, D, maxPlaces, noStart, {}, &places);
				assert(places.size() == held.size());
				for (const auto& mine : places) {
					assert((int)mine.size() <= maxPlaces);
					for (size_t k = 0; k < mine.size(); k++)
						assert(mine[k].column >= D && mine[k].column < T + D && mine[k].row > 0 && (k == 0 || mine[k - 1].row < mine[k].row));
				}
				compare(all, loop(traj.plans, places, every, tStart, noStart, {}, h, k0, T, D, R), atStart, atStop);
				compare(pipe.DeconflictWaits(held, tStart, chainPairs, false, h, D, maxPlaces, noStart), loop(traj.plans, places, chain, tStart, noStart, {}, h, k0, T, D, R), atStart, atStop);
				calls += 2;
				if (D > 0 && !barred) {
					// every vehicle with a place is committed to a wait of D / 2 steps at its first one, the others are free: the standing poses and the shift
					// behind the arrive column are what every record below depends on
					std::vector<FixedWait> stops;
					for (const auto& mine : places)
						stops.push_back(mine.empty() ? FixedWait {} : FixedWait { mine[0].row, D / 2 });
					std::vector<std::vector<WaitPlace>> listed;
					const std::vector<Wait> bound = pipe.DeconflictWaits(held, tStart, {}, true, h, D, maxPlaces, noStart, stops, &listed);
					int before = atStop;
					compare(bound, loop(traj.plans, listed, every, tStart, noStart, stops, h, k0, T, D, R), atStart, atStop);
					atFixedStop += atStop - before;
					calls++;
				}
				// the result as committed waits: every scheduled vehicle keeps its wait, clear
				std::vector<FixedWait> fixed;
				for (const Wait& w : all)
					fixed.push_back(w.status == Wait::Status::Scheduled ? FixedWait { w.place >= 0 ? w.row : -1, w.waitSteps } : FixedWait {});
				const std::vector<Wait> again = pipe.DeconflictWaits(held, tStart, {}, true, h, D, maxPlaces, noStart, fixed);
				for (size_t i = 0; i < all.size(); i++)
					if (all[i].status == Wait::Status::Scheduled) {
						assert(again[i].status == Wait::Status::Scheduled && again[i].blocker == -1 && again[i].waitSteps == all[i].waitSteps && again[i].tHold == all[i].tHold &&
							again[i].tResume == all[i].tResume && again[i].tStart == all[i].tStart);
						fedBack++;
					}
			}
		}
	}
	std::printf("%d calls compared, %d waits at the start, %d at a stop (%d of them committed), %d fed back\n", calls, atStart, atStop, atFixedStop, fedBack);
	assert(atStart >= 3 && atStop >= 1 && atFixedStop >= 1 && fedBack >= 12);
	// ---- a ticket that is not held throws; a held one without a profile is refused by the library; the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.DeconflictWaits({ held[0], held[1] }, { 0.0, 0.0 }, {}, true, Horizon(), 5, 2);
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	pipe.SpeedProfile({ held[1] }, spacing, L);
	threw = false;
	try {
		pipe.DeconflictWaits({ held[1], held[2] }, { 0.0, 0.0 }, {}, true, Horizon(), 5, 2);
	} catch (const std::exception& e) {
		threw = std::string(e.what()).find("speed_profile first") != std::string::npos;
	}
	assert(threw);
	assert(pipe.DeconflictWaits({ held[1] }, { 0.0 }, {}, true, Horizon(), 5, 2).size() == 1);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline deconflict waits: DeconflictWaits(tickets, starts) == the sequential loop over the device's poses and places\n");
	return 0;
}
