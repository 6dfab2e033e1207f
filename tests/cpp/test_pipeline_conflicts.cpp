// HybridAStarPipeline::Conflicts (pp_pipeline_conflicts) through the C++ mirror: plans are held by ticket, profiled on the device (SpeedProfile) and
// looked at for conflicts there, and every answer is compared with a plain sequential loop made here over the profile's (s, v, t) samples and the one-query
// mirror's path objects of the same plan (HybridAStar::GetGraphSearchPath): per lattice time a linear search for the sample, the position within the step
// written out from include/pp_hip.h, the edge by a walk over the lengths, the pose by the object's own Interpolate; per pair the distance of the two poses
// minus twice the validator's min_safe_radius.  Arc lengths and counts are compared exactly where the arithmetic is the same (s_enter, s_leave, first, last,
// n_present, n_times), poses and separations within 1e-9.  Then an explicit pair list, the hold flags, and a ticket without a profile.  Needs a GPU.
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

using Profiled = HybridAStarPipeline::SpeedProfiled;
using Limits = HybridAStarPipeline::SpeedLimits;
using Horizon = HybridAStarPipeline::ConflictHorizon;
using Trajectory = HybridAStarPipeline::Trajectory;
using Conflict = HybridAStarPipeline::Conflict;

Ref<Obstacle> wall(double dx, double dy, double x, double y, double theta)
{
	Ref<Obstacle> o = makeRef<Obstacle>();
	o->SetShape(makeRef<RectangleShape>(dx, dy));
	o->SetPose(Pose2d(x, y, theta));
	return o;
}

struct Plan {
	Status status = Status::Failure;
	std::vector<Pose2d> nodes;
	std::vector<Ref<PathNonHolonomicSE2Base>> edges;
};

/// where the vehicle of a profile is u seconds after its start: false if absent
bool position(const Profiled& f, double u, const Limits& L, bool holdBefore, bool holdAfter, double& s)
{
	const size_t n = f.s.size();
	if (u < 0.0) {
		s = f.s.front();
		return holdBefore;
	}
	if (u > f.t.back()) {
		s = f.s.back();
		return holdAfter;
	}
	size_t j = 0;
	for (size_t k = 0; k < n; k++) // the last sample whose time is <= u
		if (f.t[k] <= u)
			j = k;
	s = f.s[j];
	if (j + 1 == n)
		return true;
	const double ds = f.s[j + 1] - f.s[j], delta = u - f.t[j], v0 = f.v[j], v1 = f.v[j + 1];
	if (ds == 0.0)
		return true;
	const double x = ds * L.aDec / (L.aAcc + L.aDec), ta = std::sqrt(2.0 * x / L.aAcc);
	const double m = v0 + v1 > 0.0 ? (2.0 * ds) / (v0 + v1) : ta + std::sqrt(2.0 * (ds - x) / L.aDec);
	if (delta >= m)
		s = f.s[j + 1];
	else if (v0 + v1 > 0.0)
		s = f.s[j] + (v0 + (0.5 * ((v1 - v0) / m)) * delta) * delta;
	else if (delta <= ta)
		s = f.s[j] + (0.5 * L.aAcc) * delta * delta;
	else
		s = f.s[j + 1] - (0.5 * L.aDec) * (m - delta) * (m - delta);
	s = std::min(std::max(s, f.s[j]), f.s[j + 1]);
	return true;
}

Pose2d pose_at(const Plan& p, double s)
{
	if (p.edges.empty())
		return p.nodes.front();
	double before = 0.0;
	size_t e = 0;
	for (size_t k = 0; k < p.edges.size(); k++) { // the last edge that starts at or before s
		if (before <= s)
			e = k;
		before += p.edges[k]->GetLength();
	}
	before = 0.0;
	for (size_t k = 0; k < e; k++)
		before += p.edges[k]->GetLength();
	const double len = p.edges[e]->GetLength();
	return p.edges[e]->Interpolate(len > 0.0 ? std::min((s - before) / len, 1.0) : 0.0);
}

struct Loop {
	std::vector<bool> present;
	std::vector<double> s;
	std::vector<Pose2d> poses;
};

Loop loop(const Plan& p, const Profiled& f, double tStart, const Horizon& h, const Limits& L, long long k0, int T)
{
	Loop out;
	for (int m = 0; m < T; m++) {
		double s = 0.0;
		const bool here = position(f, (double)(k0 + m) * h.dt - tStart, L, h.holdBefore, h.holdAfter, s);
		out.present.push_back(here);
		out.s.push_back(s);
		out.poses.push_back(here ? pose_at(p, s) : Pose2d());
	}
	return out;
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
	HybridAStar one(params, 1, maxNodes);
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
	assert(one.Initialize(validator));
	std::vector<Plan> plans((size_t)n);
	for (int i = 0; i < n; i++) {
		one.SetInitState(starts[(size_t)i]);
		one.SetGoalState(goals[(size_t)i]);
		one.SetSeed(seeds[(size_t)i]);
		Plan& p = plans[(size_t)i];
		p.status = one.SearchPath();
		if (p.status == Status::Success) {
			p.nodes = one.GetGraphSearchNodes();
			p.edges = one.GetGraphSearchPath();
			assert(p.edges.size() + 1 == p.nodes.size());
		}
	}
	assert(plans[(size_t)n - 1].status == Status::Success && plans[(size_t)n - 1].edges.empty());
	assert(pipe.Initialize(validator));
	std::vector<uint64_t> tickets;
	assert(pipe.Submit(starts, goals, seeds, &tickets) == n);
	std::map<uint64_t, int> indexOf;
	for (int i = 0; i < n; i++)
		indexOf[tickets[(size_t)i]] = i;
	std::vector<uint64_t> held;
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<HybridAStarPipeline::Result> out;
	while ((int)held.size() < n) {
		pipe.Poll(out, 4096, true);
		for (const auto& r : out) {
			assert(r.status == plans[(size_t)indexOf.at(r.ticket)].status);
			held.push_back(r.ticket);
		}
		if (out.empty())
			std::this_thread::sleep_for(std::chrono::microseconds(200));
		assert(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(60));
	}
	const double spacing = 0.2, R = 1.0; // (the validator's min_safe_radius)
	Limits L;
	L.dwell = 0.75;
	const std::vector<Profiled> profiles = pipe.SpeedProfile(held, spacing, L);
	std::vector<double> tStart;
	for (size_t k = 0; k < held.size(); k++)
		tStart.push_back(-1.0 + 0.77 * (double)k);
	int compared = 0, conflicts = 0, apart = 0;
	for (int variant = 0; variant < 3; variant++) {
		Horizon h;
		h.tFrom = -0.5;
		h.tTo = 16.05;
		h.dt = 0.1;
		h.margin = 0.4;
		h.holdBefore = variant == 1;
		h.holdAfter = variant >= 1;
		const long long k0 = (long long)std::ceil(h.tFrom / h.dt), k1 = (long long)std::floor(h.tTo / h.dt);
		const int T = (int)(k1 - k0 + 1);
		const HybridAStarPipeline::Conflicted got = pipe.Conflicts(held, tStart, h, true);
		assert(got.plans.size() == held.size() && got.pairs.size() == held.size() * (held.size() - 1) / 2);
		std::vector<Loop> loops;
		for (size_t k = 0; k < held.size(); k++) {
			const Plan& p = plans[(size_t)indexOf.at(held[k])];
			const Trajectory& t = got.plans[k];
			if (p.status != Status::Success) {
				assert(t.status == Trajectory::Status::NoProfile && t.numPresent == 0 && t.first == -1 && t.last == -1);
				loops.push_back(Loop());
				continue;
			}
			loops.push_back(loop(p, profiles[k], tStart[k], h, L, k0, T));
			const Loop& w = loops.back();
			assert((int)t.poses.size() == T);
			int present = 0, first = -1, last = -1;
			for (int m = 0; m < T; m++) {
				if (!w.present[(size_t)m]) {
					assert(std::isnan(t.poses[(size_t)m].x()));
					continue;
				}
				present++;
				first = first < 0 ? m : first;
				last = m;
				const Pose2d &a = t.poses[(size_t)m], &b = w.poses[(size_t)m];
				if (!(std::fabs(a.x() - b.x()) <= 1e-9 && std::fabs(a.y() - b.y()) <= 1e-9 && std::fabs(std::remainder(a.theta - b.theta, 2.0 * M_PI)) <= 1e-9)) {
					std::printf("plan %zu time %d: (%.17g %.17g %.17g) on the device, (%.17g %.17g %.17g) by the loop\n", k, m, a.x(), a.y(), a.theta, b.x(), b.y(), b.theta);
					assert(false);
				}
			}
			assert(t.numPresent == present && t.first == first && t.last == last);
			assert(t.status == (present ? Trajectory::Status::Present : Trajectory::Status::NeverPresent));
			if (present)
				assert(t.sEnter == w.s[(size_t)first] && t.sLeave == w.s[(size_t)last]);
			if (h.holdBefore && h.holdAfter)
				assert(present == T);
		}
		size_t q = 0;
		for (size_t a = 0; a < held.size(); a++)
			for (size_t b = a + 1; b < held.size(); b++, q++) {
				const Conflict& c = got.pairs[q];
				if (loops[a].present.empty() || loops[b].present.empty()) {
					assert(c.status == Conflict::Status::NoProfile && c.numTimes == 0);
					continue;
				}
				int times = 0, inConflict = 0, near = 0;
				double least = HUGE_VAL, first = 0.0;
				for (int m = 0; m < T; m++) {
					if (!loops[a].present[(size_t)m] || !loops[b].present[(size_t)m])
						continue;
					const double dx = loops[a].poses[(size_t)m].x() - loops[b].poses[(size_t)m].x(), dy = loops[a].poses[(size_t)m].y() - loops[b].poses[(size_t)m].y();
					const double sep = std::sqrt(dx * dx + dy * dy) - (R + R);
					near += std::fabs(sep - h.margin) <= 1e-9;
					if (sep < h.margin && !inConflict++)
						first = (double)(k0 + m) * h.dt;
					least = std::min(least, sep);
					times++;
				}
				assert(c.numTimes == times);
				if (times == 0) {
					assert(c.status == Conflict::Status::NeverBothPresent && std::isinf(c.minSeparation));
					apart++;
					continue;
				}
				assert(std::fabs(c.minSeparation - least) <= 1e-9);
				if (near == 0) {
					assert(c.numConflict == inConflict && c.status == (inConflict ? Conflict::Status::Conflict : Conflict::Status::Free));
					assert(!inConflict || c.tFirst == first);
				}
				compared++;
				conflicts += inConflict > 0;
			}
		// the same pairs, listed backwards
		std::vector<std::pair<int, int>> listed;
		for (int a = 0; a < (int)held.size(); a++)
			for (int b = a + 1; b < (int)held.size(); b++)
				listed.insert(listed.begin(), { a, b });
		const HybridAStarPipeline::Conflicted again = pipe.Conflicts(held, tStart, listed, false, h);
		assert(again.pairs.size() == got.pairs.size() && again.plans[0].poses.empty());
		for (size_t p = 0; p < got.pairs.size(); p++) {
			const Conflict &a = again.pairs[got.pairs.size() - 1 - p], &b = got.pairs[p];
			assert(a.status == b.status && a.numTimes == b.numTimes && a.numConflict == b.numConflict && a.tFirst == b.tFirst && a.tMin == b.tMin);
			assert((a.minSeparation == b.minSeparation) && a.sMin[0] == b.sMin[0] && a.sMin[1] == b.sMin[1]);
		}
	}
	std::printf("%d pairs compared, %d in conflict, %d never both present\n", compared, conflicts, apart);
	assert(compared >= 100 && apart >= 1);
	// ---- a ticket that is not held throws; a held one without a profile is refused by the library; the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.Conflicts({ held[0], held[1] }, { 0.0, 0.0 });
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	pipe.SpeedProfile({ held[1] }, spacing, L);
	threw = false;
	try {
		pipe.Conflicts({ held[1], held[2] }, { 0.0, 0.0 });
	} catch (const std::exception& e) {
		threw = std::string(e.what()).find("speed_profile first") != std::string::npos;
	}
	assert(threw);
	assert(pipe.Conflicts({ held[1] }, { 0.0 }).plans.size() == 1);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline conflicts: Conflicts(tickets, starts) == the loop over the profile's samples and the plan's path objects\n");
	return 0;
}
