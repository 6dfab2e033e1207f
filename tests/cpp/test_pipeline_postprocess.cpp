// HybridAStarPipeline hands back what HybridAStar::SearchPath() + GetPath() hand back: queries polled with hold = true, PostProcess(tickets)
// (pp_pipeline_postprocess: sampling and smoothing on the device, by ticket), then GetPath(ticket) equals the one-query mirror's GetPath()
// pose for pose and GetSmoothingStatus(ticket) its Stats::smoothingStatus -- first with the point validator, then with a one-disc footprint
// on the validator under which at least one smoothed path leaves the footprint: Smoother::Status::Collision and the sampled path, decided
// on the host by HybridAStar and on the device by the pipeline.  Needs a GPU.
#undef NDEBUG
#include <cassert>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <thread>

#include "../../pathplanning_amd/host/map_authoring.hpp"

using namespace Planner;

namespace {

struct Want {
	Status status;
	Smoother::Status smoothing;
	std::vector<Pose2d> path, nodes;
};

bool samePoses(const std::vector<Pose2d>& a, const std::vector<Pose2d>& b)
{
	if (a.size() != b.size())
		return false;
	for (size_t i = 0; i < a.size(); i++)
		if (std::memcmp(&a[i].position.v[0], &b[i].position.v[0], 24) != 0)
			return false;
	return true;
}

} // namespace

int main()
{
	std::array<Pose2d, 2> bounds = { Pose2d(-10, -10, -M_PI), Pose2d(10, 10, M_PI) };
	Ref<StateSpaceSE2> space = makeRef<StateSpaceSE2>(bounds);
	Ref<ObstacleListOccupancyMap> map = makeRef<ObstacleListOccupancyMap>(0.1f);
	Ref<StateValidatorOccupancyMap> validator = makeRef<StateValidatorOccupancyMap>(space, map);
	const double walls[2][5] = { { 8.0, 0.6, -5.0, 1.0, 0.0 }, { 8.0, 0.6, 5.5, -2.0, 0.3 } };
	for (const auto& wl : walls) {
		Ref<Obstacle> o = makeRef<Obstacle>();
		o->SetShape(makeRef<RectangleShape>(wl[0], wl[1]));
		o->SetPose(Pose2d(wl[2], wl[3], wl[4]));
		assert(map->AddObstacle(o));
	}
	GVD(map).Update();

	const int n = 16, maxNodes = 32768;
	const float spacing = 0.8f; // interfaces/python/scripts/example.py:60
	HybridAStar::SearchParameters params;
	HybridAStar one(params, 1, maxNodes);
	one.pathInterpolation = spacing;
	HybridAStarPipeline pipe(params, n, maxNodes, 16);

	// every pass: 16 start / goal pairs valid under the validator as it is, from a fixed linear congruential sequence
	auto pass = [&](const char* name, uint64_t lcg0, int& collisions, int& smoothedOk) {
		uint64_t lcg = lcg0;
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
			seeds.push_back(7000 + (uint64_t)i);
		}
		assert(one.Initialize(validator));
		std::vector<Want> want;
		for (int i = 0; i < n; i++) {
			one.SetInitState(starts[(size_t)i]);
			one.SetGoalState(goals[(size_t)i]);
			one.SetSeed(seeds[(size_t)i]);
			Want w;
			w.status = one.SearchPath();
			w.smoothing = one.GetStats().smoothingStatus;
			w.path = one.GetPath();
			w.nodes = w.status == Status::Success ? one.GetGraphSearchNodes() : std::vector<Pose2d>();
			assert(!one.PostProcessingOverflowed());
			want.push_back(w);
		}
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
				assert(r.status == want[(size_t)indexOf.at(r.ticket)].status);
				held.push_back(r.ticket);
			}
			if (out.empty())
				std::this_thread::sleep_for(std::chrono::microseconds(200));
			assert(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(60));
		}
		assert(pipe.FreeSlots() == 0 && pipe.InFlight() == 0);
		// before PostProcess GetPath is the graph-search nodes
		for (uint64_t t : held)
			assert(samePoses(pipe.GetPath(t), want[(size_t)indexOf.at(t)].nodes) && samePoses(pipe.GetGraphSearchPath(t), want[(size_t)indexOf.at(t)].nodes));
		pipe.PostProcess(held, spacing); // in completion order, not in slot order
		int compared = 0;
		for (uint64_t t : held) {
			const Want& w = want[(size_t)indexOf.at(t)];
			if (w.status != Status::Success) {
				assert(pipe.GetPath(t).empty());
				continue;
			}
			if (pipe.GetSmoothingStatus(t) != w.smoothing || !samePoses(pipe.GetPath(t), w.path)) {
				std::printf("%s: query %d: pipeline status %d, %zu poses; HybridAStar status %d, %zu poses\n", name, indexOf.at(t), (int)pipe.GetSmoothingStatus(t),
					pipe.GetPath(t).size(), (int)w.smoothing, w.path.size());
				assert(false);
			}
			compared++;
			collisions += w.smoothing == Smoother::Status::Collision;
			smoothedOk += w.smoothing >= 0 && w.path.size() >= 5;
		}
		bool threw = false;
		pipe.Release(held);
		try {
			pipe.GetPath(held[0]);
		} catch (const std::invalid_argument&) {
			threw = true;
		}
		assert(threw && pipe.FreeSlots() == n);
		std::printf("%s: %d of %d paths compared, %d smoothed, %d Collision so far\n", name, compared, n, smoothedOk, collisions);
		return compared;
	};

	int collisions = 0, smoothedOk = 0;
	assert(pass("point validator", 12345, collisions, smoothedOk) >= 4);
	assert(collisions == 0 && smoothedOk >= 4); // Collision exists with a footprint only
	// One disc on the reference point, wider than the validator's 1 m: the search keeps the marched poses that far from the walls, the
	// smoother (which knows the 1 m only) cuts corners.  Radii are tried until a query ends Collision.  (Not the 5 m disc of
	// tests/test_gpu_pipeline_postprocess.py, which is put on plans that were searched with another footprint: HybridAStar::SearchPath
	// searches with the validator's footprint too, so here the disc has to be one the search can still plan with on a 20 m map.)
	const int before = smoothedOk;
	for (float r = 1.3f; r < 2.65f && collisions == 0; r += 0.15f) {
		validator->SetFootprint({ { 0.0, 0.0, r } });
		char name[64];
		std::snprintf(name, sizeof name, "disc (0, 0, %.2f)", (double)r);
		pass(name, 777, collisions, smoothedOk);
	}
	assert(collisions >= 1);      // at least one query whose smoothed path leaves the footprint ...
	assert(smoothedOk > before);  // ... and at least one that stays inside it, with the footprint set
	std::printf("pipeline post-processing: GetPath(ticket) == HybridAStar::GetPath() on every query\n");
	return 0;
}
