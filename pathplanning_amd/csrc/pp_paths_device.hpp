// Path value types shared by the per-path kernels (pp_paths.hip, pp_footprint.hip): the pp_rs_path record as an rs::Path,
// and PathSE2.
#pragma once

#include "../../include/pp_hip.h"
#include "pp_rs_device.hpp"

namespace ppd {

static_assert(sizeof(pp_rs_path) == 128, "pp_rs_path is a 128-byte record");

__device__ __forceinline__ rs::Path load_path(const pp_rs_path& r)
{
	rs::Path p;
	p.init = { r.start[0], r.start[1], r.start[2] };
	p.rmin = r.min_turning_radius;
	p.length = r.length;
	p.seg.length = 0.0;
	p.seg.n = 0;
#pragma unroll
	for (int i = 0; i < rs::kNumMotion; i++) {
		p.seg.len[i] = r.motion_length[i];
		p.seg.steer[i] = r.steer[i];
		p.seg.dir[i] = r.direction[i];
	}
	return p;
}

/// PathSE2, paths/path_se2.cpp:5-22
struct Se2Line {
	Pose init, fin;
	double length;
	__device__ __forceinline__ Pose interpolate(double ratio) const
	{
		Pose s;
		s.x = (1 - ratio) * init.x + ratio * fin.x;
		s.y = (1 - ratio) * init.y + ratio * fin.y;
		s.t = (1 - ratio) * init.t + ratio * fin.t; // assigned to the member: not wrapped
		return s;
	}
};

} // namespace ppd
