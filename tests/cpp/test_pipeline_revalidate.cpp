// HybridAStarPipeline::Revalidate (pp_pipeline_revalidate) through the C++ mirror: plans held by ticket are re-checked on the device against a
// map that gained a wall -- first a SECOND map (the pipeline's own untouched), then the pipeline's own map after the same edit -- and every
// verdict is compared with the one-query mirror's path objects of the same plan (HybridAStar::GetGraphSearchPath: PathConstantSteer arcs and
// the PathReedsShepp connection) marched one by one through StateValidatorOccupancyMap::IsPathValid / IsStateValid on the edited map.
// Needs a GPU.
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

using Revalidation = HybridAStarPipeline::Revalidation;

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

/// the verdict from the path objects, edge by edge, on whatever `validator`'s map holds now
Revalidation expect(const Plan& p, const Ref<StateValidatorOccupancyMap>& validator)
{
	Revalidation r;
	if (p.status != Status::Success || p.nodes.empty())
		return r; // NoPlan
	r.numEdges = (int)p.edges.size();
	for (const auto& e : p.edges)
		r.length += e->GetLength();
	r.validLength = r.length;
	r.verdict = Revalidation::Verdict::Valid;
	double before = 0.0;
	for (size_t k = 0; k < p.edges.size(); k++) {
		float last = 1.0f;
		if (!validator->IsPathValid(*p.edges[k], &last)) {
			r.verdict = Revalidation::Verdict::EdgeBlocked;
			r.blockedEdge = (int)k + 1;
			r.blockedRatio = last;
			r.validLength = before + (double)last * p.edges[k]->GetLength();
			return r;
		}
		before += p.edges[k]->GetLength();
	}
	if (!validator->IsStateValid(p.nodes.back()))
		r.verdict = Revalidation::Verdict::GoalBlocked;
	return r;
}

void same(const char* what, int q, const Revalidation& got, const Revalidation& want)
{
	const bool ok = got.verdict == want.verdict && got.numEdges == want.numEdges && got.blockedEdge == want.blockedEdge && std::fabs(got.blockedRatio - want.blockedRatio) <= 1e-6f &&
		std::fabs(got.length - want.length) <= 1e-9 && std::fabs(got.validLength - want.validLength) <= 1e-5;
	if (!ok) {
		std::printf("%s: query %d: Revalidate says verdict %d edge %d of %d ratio %.9g valid %.12g of %.12g; the path objects say verdict %d edge %d of %d ratio %.9g valid %.12g of %.12g\n",
			what, q, (int)got.verdict, got.blockedEdge, got.numEdges, (double)got.blockedRatio, got.validLength, got.length, (int)want.verdict, want.blockedEdge, want.numEdges,
			(double)want.blockedRatio, want.validLength, want.length);
		assert(false);
	}
}

} // namespace

int main()
{
	std::array<Pose2d, 2> bounds = { Pose2d(-10, -10, -M_PI), Pose2d(10, 10, M_PI) };
	Ref<StateSpaceSE2> space = makeRef<StateSpaceSE2>(bounds);
	const double walls[2][5] = { { 8.0, 0.6, -5.0, 1.0, 0.0 }, { 8.0, 0.6, 5.5, -2.0, 0.3 } };
	const double added[5] = { 9.0, 0.5, 0.5, 4.5, 1.35 }; // the wall that appears after the plans were made
	Ref<ObstacleListOccupancyMap> map = makeRef<ObstacleListOccupancyMap>(0.1f), edited = makeRef<ObstacleListOccupancyMap>(0.1f);
	Ref<StateValidatorOccupancyMap> validator = makeRef<StateValidatorOccupancyMap>(space, map), editedValidator = makeRef<StateValidatorOccupancyMap>(space, edited);
	for (const auto& wl : walls) {
		assert(map->AddObstacle(wall(wl[0], wl[1], wl[2], wl[3], wl[4])));
		assert(edited->AddObstacle(wall(wl[0], wl[1], wl[2], wl[3], wl[4])));
	}
	assert(edited->AddObstacle(wall(added[0], added[1], added[2], added[3], added[4])));
	GVD(map).Update();
	GVD(edited).Update();

	const int n = 16, maxNodes = 32768;
	HybridAStar::SearchParameters params;
	HybridAStar one(params, 1, maxNodes);
	HybridAStarPipeline pipe(params, n, maxNodes, 16);
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
		goals.push_back(validPose());
		seeds.push_back(9100 + (uint64_t)i);
	}
	// the plans as path objects, from the one-query mirror on the map as it was
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
	// the same queries held in the pipeline
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
	// on the map they were planned on every plan is still valid
	int solved = 0;
	{
		const std::vector<Revalidation> now = pipe.Revalidate(held);
		assert(now.size() == held.size());
		for (size_t k = 0; k < held.size(); k++) {
			const Plan& p = plans[(size_t)indexOf.at(held[k])];
			same("unchanged map", indexOf.at(held[k]), now[k], expect(p, validator));
			assert(p.status != Status::Success || now[k].StillValid());
			solved += p.status == Status::Success;
		}
	}
	// against the second map, which has the added wall; the pipeline's own map is untouched
	const std::vector<Revalidation> second = pipe.Revalidate(held, editedValidator);
	int blocked = 0, valid = 0;
	for (size_t k = 0; k < held.size(); k++) {
		same("second map", indexOf.at(held[k]), second[k], expect(plans[(size_t)indexOf.at(held[k])], editedValidator));
		blocked += second[k].verdict == Revalidation::Verdict::EdgeBlocked || second[k].verdict == Revalidation::Verdict::GoalBlocked;
		valid += second[k].StillValid();
	}
	std::printf("%d plans of %d queries: %d blocked by the added wall, %d still valid\n", solved, n, blocked, valid);
	assert(blocked >= 1 && valid >= 1);
	// the same wall on the pipeline's own map (nothing is in flight): Revalidate builds the fields first
	assert(map->AddObstacle(wall(added[0], added[1], added[2], added[3], added[4])));
	const std::vector<Revalidation> own = pipe.Revalidate(held);
	// (the own map's fields were updated incrementally, the second map's built in one go: each is compared with the path objects on its own map)
	int ownBlocked = 0;
	for (size_t k = 0; k < held.size(); k++) {
		same("own map, edited", indexOf.at(held[k]), own[k], expect(plans[(size_t)indexOf.at(held[k])], validator));
		ownBlocked += own[k].verdict == Revalidation::Verdict::EdgeBlocked || own[k].verdict == Revalidation::Verdict::GoalBlocked;
	}
	assert(ownBlocked >= 1);
	// a ticket that is not held throws, and the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.Revalidate({ held[0] });
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	assert(pipe.Revalidate({ held[1] }).size() == 1);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == n);
	std::printf("pipeline re-validation: Revalidate(tickets) == the path objects marched one by one, on a second map and on the edited own map\n");
	return 0;
}
