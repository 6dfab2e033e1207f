// The validator's footprint reaches the streaming pipeline (HybridAStarPipeline::Initialize / Submit -> pp_pipeline_set_footprint): with
// CAR3 on the validator, 16 queries through the pipeline give the statuses and expansion counts of HybridAStar::SearchBatch on a
// 16-query planner (the one-wave footprint kernel) with the same validator and seeds; a change of the footprint with queries in flight
// throws with the library's message.  Needs a GPU.
#undef NDEBUG
#include <cassert>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <thread>

#include "../../pathplanning_amd/host/map_authoring.hpp"

using namespace Planner;

int main()
{
	std::array<Pose2d, 2> bounds = { Pose2d(-10, -10, -M_PI), Pose2d(10, 10, M_PI) };
	Ref<StateSpaceSE2> space = makeRef<StateSpaceSE2>(bounds);
	Ref<ObstacleListOccupancyMap> map = makeRef<ObstacleListOccupancyMap>(0.1f);
	Ref<StateValidatorOccupancyMap> validator = makeRef<StateValidatorOccupancyMap>(space, map);
	// two walls: the car's three 1.3 m discs need more room around them than the reference point's 1 m
	const double walls[2][5] = { { 8.0, 0.6, -5.0, 1.0, 0.0 }, { 8.0, 0.6, 5.5, -2.0, 0.3 } };
	for (const auto& wl : walls) {
		Ref<Obstacle> o = makeRef<Obstacle>();
		o->SetShape(makeRef<RectangleShape>(wl[0], wl[1]));
		o->SetPose(Pose2d(wl[2], wl[3], wl[4]));
		assert(map->AddObstacle(o));
	}
	GVD(map).Update();
	const std::vector<FootprintDisc> car3 = { { -0.2, 0.0, 1.3f }, { 1.4, 0.0, 1.3f }, { 3.0, 0.0, 1.3f } };
	validator->SetFootprint(car3);

	// 16 start / goal pairs that are valid for the car, from a fixed linear congruential sequence
	const int n = 16;
	uint64_t lcg = 12345;
	auto uniform = [&](double lo, double hi) {
		lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
		return lo + (hi - lo) * (double)(lcg >> 11) / 9007199254740992.0;
	};
	auto validPose = [&]() {
		for (;;) {
			const Pose2d p(uniform(-9.0, 9.0), uniform(-9.0, 9.0), uniform(-M_PI, M_PI));
			if (validator->IsStateValid(p))
				return p;
		}
	};
	std::vector<Pose2d> starts, goals;
	std::vector<uint64_t> seeds;
	for (int i = 0; i < n; i++) {
		starts.push_back(validPose());
		goals.push_back(validPose());
		seeds.push_back(4000 + (uint64_t)i);
	}

	const int maxNodes = 32768;
	HybridAStar::SearchParameters params;
	HybridAStar batch(params, n, maxNodes);
	assert(batch.Initialize(validator));
	const std::vector<pp_query_result> want = batch.SearchBatch(starts, goals, seeds);

	HybridAStarPipeline pipe(params, n, maxNodes, 16);
	assert(pipe.Initialize(validator));
	auto submit = [&]() {
		std::vector<uint64_t> tickets;
		assert(pipe.Submit(starts, goals, seeds, &tickets) == n);
		std::map<uint64_t, int> indexOf;
		for (int i = 0; i < n; i++)
			indexOf[tickets[(size_t)i]] = i;
		return indexOf;
	};
	auto drain = [&](const std::map<uint64_t, int>& indexOf, std::vector<HybridAStarPipeline::Result>& byQuery) {
		byQuery.assign((size_t)n, HybridAStarPipeline::Result());
		int got = 0;
		const auto t0 = std::chrono::steady_clock::now();
		std::vector<HybridAStarPipeline::Result> out;
		while (got < n) {
			pipe.Poll(out);
			for (const auto& r : out)
				byQuery[(size_t)indexOf.at(r.ticket)] = r, got++;
			if (out.empty())
				std::this_thread::sleep_for(std::chrono::microseconds(200));
			assert(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(60));
		}
	};
	std::vector<HybridAStarPipeline::Result> car;
	auto indexOf = submit();
	drain(indexOf, car);
	int solved = 0;
	for (int i = 0; i < n; i++) {
		assert((car[(size_t)i].status == Status::Success) == (want[(size_t)i].status == 0));
		assert(car[(size_t)i].numExpanded == want[(size_t)i].n_expanded);
		assert(car[(size_t)i].numPathNodes == want[(size_t)i].n_path);
		solved += want[(size_t)i].status == 0;
	}
	assert(solved >= 4);

	// the footprint changes with queries in flight: Submit throws with the library's message, the queries in flight finish as they were
	indexOf = submit();
	validator->ClearFootprint();
	bool threw = false;
	try {
		pipe.Submit(starts, goals, seeds);
	} catch (const std::exception& e) {
		threw = std::strstr(e.what(), "in flight") != nullptr;
	}
	assert(threw);
	drain(indexOf, car);
	int differ = 0;
	for (int i = 0; i < n; i++)
		assert(car[(size_t)i].numExpanded == want[(size_t)i].n_expanded);
	// ... and once they are polled the cleared footprint is accepted: the point validator's searches
	const std::vector<pp_query_result> point = batch.SearchBatch(starts, goals, seeds);
	indexOf = submit();
	drain(indexOf, car);
	for (int i = 0; i < n; i++) {
		assert(car[(size_t)i].numExpanded == point[(size_t)i].n_expanded);
		differ += point[(size_t)i].n_expanded != want[(size_t)i].n_expanded;
	}
	assert(differ >= 1); // the footprint mattered on this map
	std::printf("pipeline footprint: %d of %d solved with the car, %d searches differ from the point validator's\n", solved, n, differ);
	return 0;
}
