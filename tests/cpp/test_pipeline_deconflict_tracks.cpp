// HybridAStarPipeline::DeconflictTracks (pp_pipeline_deconflict_tracks) through the C++ mirror: plans are held by ticket, profiled on the device
// (SpeedProfile) and given start delays there that also clear tracked movers, and every record is compared with a plain sequential loop made here over
// the device's own poses and the tracks' waypoints.  Conflicts(..., withPoses) over the horizon that begins max_delay_steps lattice steps earlier
// returns the extended trajectory, a delay is an index shift in it, a track's position is the header's interpolation written out, and the loop below --
// vehicles in index order, delays ascending, times ascending, partners ascending and the tracks behind them -- is the rule of include/pp_hip.h.  The
// separations are formed in the header's order and without contraction, so status, delay, candidates tried, blocker, effective start and the
// blocker's time are compared EXACTLY, and so are the counts, times and smallest separation of every (vehicle, track) record.  Then no tracks at all
// (Deconflict's records), the plain check (no pairs, a largest delay of zero), and a track set the library refuses.  Needs a GPU.
#undef NDEBUG
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <limits>
#include <thread>

#include "../../pathplanning_amd/host/map_authoring.hpp"

using namespace Planner;

namespace {

using Limits = HybridAStarPipeline::SpeedLimits;
using Horizon = HybridAStarPipeline::ConflictHorizon;
using Delay = HybridAStarPipeline::Delay;
using Track = HybridAStarPipeline::Track;
using TrackConflict = HybridAStarPipeline::TrackConflict;

Ref<Obstacle> wall(double dx, double dy, double x, double y, double theta)
{
	Ref<Obstacle> o = makeRef<Obstacle>();
	o->SetShape(makeRef<RectangleShape>(dx, dy));
	o->SetPose(Pose2d(x, y, theta));
	return o;
}

/// where a track is at tau (false: absent), by a linear search
bool trackAt(const Track& k, double tau, double& x, double& y)
{
	const auto& w = k.waypoints;
	if (tau < w.front().t || tau > w.back().t)
		return false;
	size_t j = 0;
	while (j + 1 < w.size() && w[j + 1].t <= tau)
		j++;
	if (j + 1 == w.size()) {
		x = w[j].x;
		y = w[j].y;
		return true;
	}
	const double lam = (tau - w[j].t) / (w[j + 1].t - w[j].t);
	x = w[j].x + lam * (w[j + 1].x - w[j].x);
	y = w[j].y + lam * (w[j + 1].y - w[j].y);
	return true;
}

struct Expected {
	int status = -1, delay = -1, tried = 0, blocker = -1;
	double tStart = 0.0, tBlock = 0.0;
	struct Against {
		int status = -1, times = 0, conflicts = 0;
		double tFirst = 0.0, minSeparation = 0.0, tMin = 0.0;
	};
	std::vector<Against> tracks;
};

/// the rule, one vehicle after the other; poses[i] holds T + D columns, NaN where absent; below[i]: the partners of smaller index
std::vector<Expected> loop(const std::vector<HybridAStarPipeline::Trajectory>& plans, const std::vector<std::vector<int>>& below, const std::vector<double>& tStart,
	const std::vector<Track>& tracks, const Horizon& h, long long k0, int T, int D, double R)
{
	const size_t n = plans.size(), M = tracks.size();
	std::vector<Expected> out(n);
	for (size_t i = 0; i < n; i++) {
		Expected& e = out[i];
		e.tracks.resize(M);
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
				for (size_t k = 0; k < M && mHit < 0; k++) { // (a track is partner n + k: behind every vehicle at this time)
					double x, y;
					if (!trackAt(tracks[k], (double)(k0 + m) * h.dt, x, y))
						continue;
					const double dx = a.x() - x, dy = a.y() - y;
					if (std::sqrt(dx * dx + dy * dy) - (R + tracks[k].radius) < h.margin) {
						mHit = m;
						jHit = (int)(n + k);
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
		const int candidate = e.delay >= 0 ? e.delay : D; // the reported candidate
		for (size_t k = 0; k < M; k++) {
			Expected::Against& g = e.tracks[k];
			g.minSeparation = std::numeric_limits<double>::infinity();
			for (int m = 0; m < T; m++) {
				const Pose2d& a = plans[i].poses[(size_t)(m + D - candidate)];
				const double tau = (double)(k0 + m) * h.dt;
				double x, y;
				if (std::isnan(a.x()) || !trackAt(tracks[k], tau, x, y))
					continue;
				const double dx = a.x() - x, dy = a.y() - y, sep = std::sqrt(dx * dx + dy * dy) - (R + tracks[k].radius);
				g.times++;
				if (sep < h.margin && g.conflicts++ == 0)
					g.tFirst = tau;
				if (sep < g.minSeparation) {
					g.minSeparation = sep;
					g.tMin = tau;
				}
			}
			g.status = g.times == 0 ? 2 : (g.conflicts > 0 ? 1 : 0);
			if (g.times == 0)
				g.tMin = 0.0;
		}
	}
	return out;
}

struct Tally {
	int waited = 0, byTrack = 0, byVehicle = 0;
};

void compare(const HybridAStarPipeline::DelayedWithTracks& got, const std::vector<Expected>& want, size_t M, Tally& tally)
{
	assert(got.plans.size() == want.size() && got.tracks.size() == want.size());
	const int n = (int)want.size();
	for (size_t i = 0; i < want.size(); i++) {
		const Delay& g = got.plans[i];
		const Expected& w = want[i];
		if (!((int)g.status == w.status && g.delaySteps == w.delay && g.numTried == w.tried && g.blocker == w.blocker && g.tStart == w.tStart && g.tBlock == w.tBlock)) {
			std::printf("vehicle %zu: (%d %d %d %d %.17g %.17g) on the device, (%d %d %d %d %.17g %.17g) by the loop\n", i, (int)g.status, g.delaySteps, g.numTried, g.blocker,
				g.tStart, g.tBlock, w.status, w.delay, w.tried, w.blocker, w.tStart, w.tBlock);
			assert(false);
		}
		assert(g.blocker >= 0 || (g.tBlock == 0.0 && g.sBlock[0] == 0.0 && g.sBlock[1] == 0.0));
		assert(g.blocker < n || g.sBlock[1] == 0.0);
		tally.waited += g.delaySteps > 0;
		tally.byTrack += g.blocker >= n;
		tally.byVehicle += g.blocker >= 0 && g.blocker < n;
		assert(got.tracks[i].size() == M);
		for (size_t k = 0; k < M; k++) {
			const TrackConflict& c = got.tracks[i][k];
			const Expected::Against& a = w.tracks[k];
			if (w.status < 0) {
				assert((int)c.status == -1 && c.numTimes == 0 && c.minSeparation == 0.0);
				continue;
			}
			if (!((int)c.status == a.status && c.numTimes == a.times && c.numConflict == a.conflicts && c.tFirst == a.tFirst && c.minSeparation == a.minSeparation && c.tMin == a.tMin)) {
				std::printf("vehicle %zu, track %zu: (%d %d %d %.17g %.17g %.17g) on the device, (%d %d %d %.17g %.17g %.17g) by the loop\n", i, k, (int)c.status, c.numTimes,
					c.numConflict, c.tFirst, c.minSeparation, c.tMin, a.status, a.times, a.conflicts, a.tFirst, a.minSeparation, a.tMin);
				assert(false);
			}
			assert((int)g.status != 0 || a.status != 1); // a scheduled vehicle is clear of every track
		}
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
	std::vector<std::vector<int>> every(held.size()), chain(held.size()), nobody(held.size());
	std::vector<std::pair<int, int>> chainPairs;
	for (int i = 0; i < (int)held.size(); i++) {
		for (int j = 0; j < i; j++)
			every[(size_t)i].push_back(j);
		if (i > 0) {
			chain[(size_t)i].push_back(i - 1);
			chainPairs.push_back(i % 2 ? std::make_pair(i, i - 1) : std::make_pair(i - 1, i));
		}
	}
	// the movers: crossers between start and goal poses, standers at goals for a part and for the whole of the horizon, one waypoint on a lattice time
	std::vector<Track> tracks;
	for (int k = 0; k < 9; k++) {
		Track t;
		t.radius = k % 3 == 0 ? 0.0 : (k % 3 == 1 ? 0.3 : 1.0);
		const Pose2d &a = starts[(size_t)k], &b = goals[(size_t)((k + 5) % n)], &g = goals[(size_t)k];
		if (k % 4 == 0)
			t.waypoints = { { 0.07 + (double)k, a.x(), a.y() }, { 3.3 + (double)k, b.x(), b.y() }, { 6.1 + (double)k, g.x(), g.y() } };
		else if (k % 4 == 1)
			t.waypoints = { { 2.05, g.x(), g.y() }, { 6.45, g.x(), g.y() } };
		else if (k % 4 == 2)
			t.waypoints = { { -1.0, g.x(), g.y() }, { 100.0, g.x(), g.y() } };
		else
			t.waypoints = { { (double)(20 + k) * 0.1, a.x(), a.y() } };
		tracks.push_back(t);
	}
	Tally tally;
	int calls = 0;
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
			compare(pipe.DeconflictTracks(held, tStart, tracks, {}, true, h, D), loop(traj.plans, every, tStart, tracks, h, k0, T, D, R), tracks.size(), tally);
			compare(pipe.DeconflictTracks(held, tStart, tracks, chainPairs, false, h, D), loop(traj.plans, chain, tStart, tracks, h, k0, T, D, R), tracks.size(), tally);
			compare(pipe.DeconflictTracks(held, tStart, tracks, {}, false, h, D), loop(traj.plans, nobody, tStart, tracks, h, k0, T, D, R), tracks.size(), tally);
			calls += 3;
			// no tracks: Deconflict's records; without details: the same plans and no track records
			const auto none = pipe.DeconflictTracks(held, tStart, {}, chainPairs, false, h, D);
			const auto plain = pipe.Deconflict(held, tStart, chainPairs, false, h, D);
			assert(none.plans.size() == plain.size() && none.tracks.size() == plain.size() && none.tracks[0].empty());
			for (size_t i = 0; i < plain.size(); i++)
				assert(none.plans[i].status == plain[i].status && none.plans[i].delaySteps == plain[i].delaySteps && none.plans[i].blocker == plain[i].blocker &&
					none.plans[i].tStart == plain[i].tStart && none.plans[i].tBlock == plain[i].tBlock && none.plans[i].sBlock[1] == plain[i].sBlock[1]);
			const auto brief = pipe.DeconflictTracks(held, tStart, tracks, chainPairs, false, h, D, false);
			assert(brief.tracks.empty() && brief.plans.size() == held.size());
		}
	}
	std::printf("%d calls compared, %d vehicles waited, %d blocked by a track, %d by a vehicle\n", calls, tally.waited, tally.byTrack, tally.byVehicle);
	assert(tally.waited >= 3 && tally.byTrack >= 3 && tally.byVehicle >= 1);
	// ---- a track set the library refuses throws and names the offender; the pipeline goes on
	bool threw = false;
	try {
		std::vector<Track> bad = tracks;
		bad[2].waypoints[1].t = bad[2].waypoints[0].t;
		pipe.DeconflictTracks(held, tStart, bad, {}, true, Horizon(), 5);
	} catch (const std::exception& e) {
		threw = std::string(e.what()).find("of track 2") != std::string::npos;
	}
	assert(threw);
	threw = false;
	try {
		pipe.DeconflictTracks({ held[0], 123456789 }, { 0.0, 0.0 }, tracks, {}, true, Horizon(), 5);
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	assert(pipe.DeconflictTracks({ held[1] }, { 0.0 }, tracks, {}, true, Horizon(), 5).plans.size() == 1);
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline deconflict tracks: DeconflictTracks(tickets, starts, tracks) == the sequential loop over the device's poses\n");
	return 0;
}
