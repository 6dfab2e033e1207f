// HybridAStarPipeline::Deconflict (pp_pipeline_deconflict) through the C++ mirror: plans are held by ticket, profiled on the device (SpeedProfile) and
// given start delays there, and every record is compared with a plain sequential loop made here over the device's own poses: Conflicts(..., withPoses)
// over the horizon that begins max_delay_steps lattice steps earlier returns the extended trajectory, a delay is an index shift in it, and the loop
// below -- vehicles in index order, delays ascending, times ascending, partners ascending -- is the rule of include/pp_hip.h written out.  The
// separation is the distance of the two poses minus twice the validator's min_safe_radius, in the header's order and without contraction, so status,
// delay, candidates tried, blocker, effective start and the blocker's time are compared EXACTLY.  Then an explicit pair list (a chain), a largest
// delay of zero, and a ticket without a profile.  Needs a GPU.
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
using Delay = HybridAStarPipeline::Delay;

Ref<Obstacle> wall(double dx, double dy, double x, double y, double theta)
{
	Ref<Obstacle> o = makeRef<Obstacle>();
	o->SetShape(makeRef<RectangleShape>(dx, dy));
	o->SetPose(Pose2d(x, y, theta));
	return o;
}

struct Expected {
	int status = -1, delay = -1, tried = 0, blocker = -1;
	double tStart = 0.0, tBlock = 0.0;
};

/// the rule, one vehicle after the other; poses[i] holds T + D columns, NaN where absent; below[i]: the partners of smaller index
std::vector<Expected> loop(const std::vector<HybridAStarPipeline::Trajectory>& plans, const std::vector<std::vector<int>>& below, const std::vector<double>& tStart,
	const Horizon& h, long long k0, int T, int D, double R)
{
	const size_t n = plans.size();
	std::vector<Expected> out(n);
	for (size_t i = 0; i < n; i++) {
		Expected& e = out[i];
		if (plans[i].status == HybridAStarPipeline::Trajectory::Status::NoProfile)
			continue;
		for (int d = 0; d <= D && e.delay < 0; d++) {
			int mHit = -1, jHit = -1;
			for (int m = 0; m < T && mHit < 0; m++) {
				const Pose2d& a = plans[i].poses[(size_t)(m + D - d)];
				if (std::isnan(a.x()))
					continue;
				for (int j : below[i]) {
					if (out[(size_t)j].delay < 0 || (jHit >= 0 && j >= jHit))
						continue;
					const Pose2d& b = plans[(size_t)j].poses[(size_t)(m + D - out[(size_t)j].delay)];
					if (std::isnan(b.x()))
						continue;
					const double dx = a.x() - b.x(), dy = a.y() - b.y();
					if (std::sqrt(dx * dx + dy * dy) - (R + R) < h.margin) {
						mHit = m;
						jHit = j;
					}
				}
			}
			e.tried++;
			if (mHit < 0) {
				e.delay = d;
				break;
			}
			e.blocker = jHit;
			e.tBlock = (double)(k0 + mHit) * h.dt;
		}
		e.status = e.delay >= 0 ? 0 : 1;
		e.tStart = e.delay >= 0 ? tStart[i] + (double)e.delay * h.dt : tStart[i];
	}
	return out;
}

int compare(const std::vector<Delay>& got, const std::vector<Expected>& want)
{
	assert(got.size() == want.size());
	int waited = 0;
	for (size_t i = 0; i < got.size(); i++) {
		const Delay& g = got[i];
		const Expected& w = want[i];
		if (!((int)g.status == w.status && g.delaySteps == w.delay && g.numTried == w.tried && g.blocker == w.blocker && g.tStart == w.tStart && g.tBlock == w.tBlock)) {
			std::printf("vehicle %zu: (%d %d %d %d %.17g %.17g) on the device, (%d %d %d %d %.17g %.17g) by the loop\n", i, (int)g.status, g.delaySteps, g.numTried, g.blocker,
				g.tStart, g.tBlock, w.status, w.delay, w.tried, w.blocker, w.tStart, w.tBlock);
			assert(false);
		}
		assert(g.blocker >= 0 || (g.tBlock == 0.0 && g.sBlock[0] == 0.0 && g.sBlock[1] == 0.0));
		assert(g.sBlock[0] >= 0.0 && g.sBlock[1] >= 0.0);
		waited += g.delaySteps > 0;
	}
	return waited;
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
	int waited = 0, calls = 0;
	for (int variant = 0; variant < 3; variant++) {
		Horizon h;
		h.tFrom = 0.0;
		h.tTo = 14.05;
		h.dt = 0.1;
		h.margin = 1.0;
		h.holdBefore = variant == 1;
		h.holdAfter = variant >= 1;
		for (int D : { 0, 70 }) {
			const long long k0 = (long long)std::ceil(h.tFrom / h.dt), k1 = (long long)std::floor(h.tTo / h.dt);
			const int T = (int)(k1 - k0 + 1);
			Horizon extended = h; // the lattice indices k0 - D .. k1: half a step before the first one
			extended.tFrom = ((double)(k0 - D) - 0.5) * h.dt;
			const HybridAStarPipeline::Conflicted traj = pipe.Conflicts(held, tStart, extended, true);
			assert(traj.plans.size() == held.size() && (int)traj.plans[0].poses.size() == T + D);
			waited += compare(pipe.Deconflict(held, tStart, {}, true, h, D), loop(traj.plans, every, tStart, h, k0, T, D, R));
			waited += compare(pipe.Deconflict(held, tStart, chainPairs, false, h, D), loop(traj.plans, chain, tStart, h, k0, T, D, R));
			calls += 2;
		}
	}
	std::printf("%d calls compared, %d vehicles waited\n", calls, waited);
	assert(waited >= 3);
	// ---- a ticket that is not held throws; a held one without a profile is refused by the library; the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.Deconflict({ held[0], held[1] }, { 0.0, 0.0 }, {}, true, Horizon(), 5);
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	pipe.SpeedProfile({ held[1] }, spacing, L);
	threw = false;
	try {
		pipe.Deconflict({ held[1], held[2] }, { 0.0, 0.0 }, {}, true, Horizon(), 5);
	} catch (const std::exception& e) {
		threw = std::string(e.what()).find("speed_profile first") != std::string::npos;
	}
	assert(threw);
	assert(pipe.Deconflict({ held[1] }, { 0.0 }, {}, true, Horizon(), 5).size() == 1);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline deconflict: Deconflict(tickets, starts) == the sequential loop over the device's poses\n");
	return 0;
}
