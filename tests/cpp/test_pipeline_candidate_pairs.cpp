// HybridAStarPipeline::CandidatePairs (pp_pipeline_candidate_pairs) through the C++ mirror: plans are held by ticket, profiled on the device
// (SpeedProfile) and boxed and paired there, and the list is compared with a plain sequential loop made here over the device's own poses:
// Conflicts(..., withPoses) over the horizon that begins max_delay_steps lattice steps earlier returns the extended trajectory, and the loop below --
// plans in index order, boxes ascending, columns ascending, then every pair i < j with the boxes ascending -- is the rule of include/pp_hip.h written
// out.  Boxes are min and max of the device's doubles and the test is a subtraction and a comparison, so the list, the first box of every pair, the
// counts, the reach and the boxes are compared EXACTLY.  Then: the list cut at maxPairs is the head of the whole list; Deconflict over the list gives
// the records of Deconflict over every pair; a ticket without a profile.  Needs a GPU.
#undef NDEBUG
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

#include "../../pathplanning_amd/host/map_authoring.hpp"

using namespace Planner;

namespace {

using Limits = HybridAStarPipeline::SpeedLimits;
using Horizon = HybridAStarPipeline::ConflictHorizon;
using Candidates = HybridAStarPipeline::Candidates;
using Delay = HybridAStarPipeline::Delay;

Ref<Obstacle> wall(double dx, double dy, double x, double y, double theta)
{
	Ref<Obstacle> o = makeRef<Obstacle>();
	o->SetShape(makeRef<RectangleShape>(dx, dy));
	o->SetPose(Pose2d(x, y, theta));
	return o;
}

bool sameBits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }

/// the rule; poses of T + D columns per plan, NaN where absent (an empty vector: no profile)
Candidates loop(const std::vector<HybridAStarPipeline::Trajectory>& plans, const Horizon& h, int T, int D, int B, double R)
{
	const size_t n = plans.size();
	const int NB = (T + B - 1) / B;
	const double none = std::nan("");
	Candidates out;
	out.numBoxes = NB;
	out.reach = (h.margin + (R + R)) + 1e-6;
	out.boxes.assign(n, std::vector<Candidates::Box>((size_t)NB, Candidates::Box { none, none, none, none }));
	for (size_t i = 0; i < n; i++) {
		bool any = false;
		for (int b = 0; b < NB && !plans[i].poses.empty(); b++) {
			Candidates::Box& box = out.boxes[i][(size_t)b];
			for (int c = b * B; c <= std::min(b * B + B, T) - 1 + D; c++) {
				const Pose2d& p = plans[i].poses[(size_t)c];
				if (std::isnan(p.x()))
					continue;
				if (std::isnan(box.xMin))
					box = Candidates::Box { p.x(), p.y(), p.x(), p.y() };
				box.xMin = std::min(box.xMin, p.x());
				box.yMin = std::min(box.yMin, p.y());
				box.xMax = std::max(box.xMax, p.x());
				box.yMax = std::max(box.yMax, p.y());
				any = true;
			}
		}
		out.numBoxed += any;
	}
	for (size_t i = 0; i < n; i++)
		for (size_t j = i + 1; j < n; j++)
			for (int b = 0; b < NB; b++) {
				const Candidates::Box &p = out.boxes[i][(size_t)b], &q = out.boxes[j][(size_t)b];
				if (std::isnan(p.xMin) || std::isnan(q.xMin))
					continue;
				const double gx = std::max(p.xMin - q.xMax, q.xMin - p.xMax), gy = std::max(p.yMin - q.yMax, q.yMin - p.yMax);
				if (!(gx > out.reach) && !(gy > out.reach)) {
					out.pairs.emplace_back((int)i, (int)j);
					out.firstBox.push_back(b);
					break;
				}
			}
	out.numFound = (long long)out.pairs.size();
	return out;
}

void compare(const Candidates& got, const Candidates& want, bool boxes)
{
	if (!(got.pairs == want.pairs && got.firstBox == want.firstBox && got.numFound == want.numFound && got.numBoxes == want.numBoxes && got.numBoxed == want.numBoxed &&
			sameBits(got.reach, want.reach))) {
		std::printf("%zu pairs (%lld found, %d boxes, %d boxed, reach %.17g) on the device, %zu (%lld, %d, %d, %.17g) by the loop\n", got.pairs.size(), got.numFound, got.numBoxes,
			got.numBoxed, got.reach, want.pairs.size(), want.numFound, want.numBoxes, want.numBoxed, want.reach);
		assert(false);
	}
	if (!boxes)
		return;
	assert(got.boxes.size() == want.boxes.size());
	for (size_t i = 0; i < got.boxes.size(); i++) {
		assert(got.boxes[i].size() == want.boxes[i].size());
		for (size_t b = 0; b < got.boxes[i].size(); b++) {
			const Candidates::Box &g = got.boxes[i][b], &w = want.boxes[i][b];
			assert(sameBits(g.xMin, w.xMin) && sameBits(g.yMin, w.yMin) && sameBits(g.xMax, w.xMax) && sameBits(g.yMax, w.yMax));
		}
	}
}

bool sameRecords(const std::vector<Delay>& a, const std::vector<Delay>& b)
{
	if (a.size() != b.size())
		return false;
	for (size_t i = 0; i < a.size(); i++)
		if (!(a[i].status == b[i].status && a[i].delaySteps == b[i].delaySteps && a[i].numTried == b[i].numTried && a[i].blocker == b[i].blocker && a[i].tStart == b[i].tStart &&
				a[i].tBlock == b[i].tBlock && a[i].sBlock[0] == b[i].sBlock[0] && a[i].sBlock[1] == b[i].sBlock[1]))
			return false;
	return true;
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
	int calls = 0;
	size_t fewest = (size_t)-1, most = 0;
	for (int variant = 0; variant < 3; variant++) {
		Horizon h;
		h.tFrom = 0.0;
		h.tTo = 14.05;
		h.dt = 0.1;
		h.margin = variant == 2 ? 0.0 : 1.0;
		h.holdBefore = variant == 1;
		h.holdAfter = variant >= 1;
		for (int D : { 0, 70 }) {
			const long long k0 = (long long)std::ceil(h.tFrom / h.dt), k1 = (long long)std::floor(h.tTo / h.dt);
			const int T = (int)(k1 - k0 + 1);
			Horizon extended = h; // the lattice indices k0 - D .. k1: half a step before the first one
			extended.tFrom = ((double)(k0 - D) - 0.5) * h.dt;
			const HybridAStarPipeline::Conflicted traj = pipe.Conflicts(held, tStart, extended, true);
			assert(traj.plans.size() == held.size() && (int)traj.plans[0].poses.size() == T + D);
			const std::vector<Delay> everyPair = pipe.Deconflict(held, tStart, {}, true, h, D);
			for (int B : { 1, 16, 64, T }) {
				const Candidates want = loop(traj.plans, h, T, D, B, R);
				const Candidates got = pipe.CandidatePairs(held, tStart, h, B, D, -1, true);
				compare(got, want, true);
				fewest = std::min(fewest, got.pairs.size());
				most = std::max(most, got.pairs.size());
				// cut at maxPairs: the head of the list, and the whole count
				const int cut = (int)got.pairs.size() / 2;
				const Candidates head = pipe.CandidatePairs(held, tStart, h, B, D, cut);
				assert(head.numFound == got.numFound && (int)head.pairs.size() == cut && std::equal(head.pairs.begin(), head.pairs.end(), got.pairs.begin()) &&
					std::equal(head.firstBox.begin(), head.firstBox.end(), got.firstBox.begin()));
				// the guarantee: the delay call over the list is the delay call over every pair
				assert(sameRecords(pipe.Deconflict(held, tStart, got.pairs, false, h, D), everyPair));
				calls++;
			}
		}
	}
	std::printf("%d calls compared, lists of %zu .. %zu of %d pairs\n", calls, fewest, most, n * (n - 1) / 2);
	assert(fewest > 0 && most <= (size_t)(n * (n - 1) / 2)); // (12 vehicles of radius 1 in a 20 m box: how much the list leaves out is printed, not asserted)
	// ---- a ticket that is not held throws; a held one without a profile is refused by the library; the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.CandidatePairs({ held[0], held[1] }, { 0.0, 0.0 }, Horizon());
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	pipe.SpeedProfile({ held[1] }, spacing, L);
	threw = false;
	try {
		pipe.CandidatePairs({ held[1], held[2] }, { 0.0, 0.0 }, Horizon());
	} catch (const std::exception& e) {
		threw = std::string(e.what()).find("speed_profile first") != std::string::npos;
	}
	assert(threw);
	const Candidates one = pipe.CandidatePairs({ held[1] }, { 0.0 }, Horizon());
	assert(one.pairs.empty() && one.numFound == 0 && one.numBoxes == 10 && one.numBoxed <= 1);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline candidate pairs: CandidatePairs(tickets, starts) == the sequential loop over the device's poses\n");
	return 0;
}
