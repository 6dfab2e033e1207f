// Vehicle footprint (include/pp_hip.h, "vehicle footprint"): K discs in the vehicle frame instead of the one look-up at
// the pose's reference point.  Batched kernels (gfx950), the device arithmetic is pp_footprint_device.hpp's:
//   check_states_footprint        general form: any batch, any alignment, optional clearance; reads the float distance grid
//   check_states_footprint_pipe   streamed form of k_check_states_pipe over the footprint's validity bitmaps (one per distinct radius),
//                                 read through the cache (an LDS-resident form like k_check_states_lds is not shipped: it has not been
//                                 measured against this one)
//   check_arcs_footprint / check_rs_paths_footprint / check_se2_paths_footprint   the march of IsPathValid, one lane per path
// and the pp_footprint object: bound to one map, its bitmaps follow the map's distance grid (pp_map::distVersion).
#include "pp_internal.hpp"

#include <cmath>
#include <memory>

#include "pp_paths_device.hpp"

using namespace ppd;
using pph::set_error;

namespace {

constexpr int kBlock = 256;

inline int grid_for(int64_t n, int block, int maxBlocks = 256 * 16)
{
	int64_t b = (n + block - 1) / block;
	if (b < 1)
		b = 1;
	if (b > maxBlocks)
		b = maxBlocks;
	return (int)b;
}

// ------------------------------------------------------------ check_states --
// One pose per thread against the float grid: ragged tails, unaligned views, small batches, and every call that wants the
// clearance (min_i (d_i - r_i), which the bitmaps do not hold; -1 where the pose is invalid).
__global__ void __launch_bounds__(kBlock) k_check_states_footprint(MapView m, Footprint fp, int64_t n, const double* __restrict__ poses, uint8_t* __restrict__ valid,
	float* __restrict__ clearance)
{
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
		float clear = 0.0f, border = 0.0f;
		const bool ok = fp_state_valid(m, fp, poses[3 * i], poses[3 * i + 1], poses[3 * i + 2], clear, border);
		valid[i] = ok ? 1 : 0;
		if (clearance)
			clearance[i] = ok ? clear : -1.0f;
	}
}

// The streamed form for large aligned batches: k_check_states_pipe's tile pipeline (next tile's loads in registers while this one
// is evaluated, non-temporal pose stream, four flags per 32-bit word on the way out) around the footprint's predicate: one sincos
// per pose and one bit look-up per disc.
constexpr int kPer = 4;
typedef double dvec2 __attribute__((ext_vector_type(2)));
__global__ void __launch_bounds__(kBlock) k_check_states_footprint_pipe(MapView m, Footprint fp, const uint32_t* __restrict__ bits, uint32_t wordsPer, int64_t nTiles,
	const dvec2* __restrict__ src, uint32_t* __restrict__ valid4)
{
	constexpr int kTile = kBlock * kPer;
	constexpr int kVec = kPer * 3 / 2;
	static_assert(kPer == 4, "four flags per 32-bit word");
	__shared__ dvec2 tile[kTile * 3 / 2];
	__shared__ uint8_t flags[2][kTile];
	dvec2 v[kVec];
	int64_t tileIdx = blockIdx.x;
	if (tileIdx < nTiles) {
		const dvec2* s2 = src + tileIdx * (kTile * 3 / 2);
#pragma unroll
		for (int k = 0; k < kVec; k++)
			v[k] = __builtin_nontemporal_load(&s2[k * kBlock + threadIdx.x]);
	}
	int par = 0;
	for (; tileIdx < nTiles; tileIdx += gridDim.x, par ^= 1) {
#pragma unroll
		for (int k = 0; k < kVec; k++)
			tile[k * kBlock + threadIdx.x] = v[k];
		__syncthreads();
		const int64_t next = tileIdx + gridDim.x;
		if (next < nTiles) {
			const dvec2* s2 = src + next * (kTile * 3 / 2);
#pragma unroll
			for (int k = 0; k < kVec; k++)
				v[k] = __builtin_nontemporal_load(&s2[k * kBlock + threadIdx.x]);
		}
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			const int i = k * kBlock + threadIdx.x;
			const double* t = reinterpret_cast<const double*>(tile) + 3 * i;
			flags[par][i] = fp_state_valid_bits_flat(m, fp, t[0], t[1], t[2], bits, wordsPer) ? 1 : 0;
		}
		__syncthreads();
		__builtin_nontemporal_store(reinterpret_cast<const uint32_t*>(flags[par])[threadIdx.x], &valid4[tileIdx * (kTile / 4) + threadIdx.x]);
	}
}

// ------------------------------------------------------------- path checks --
// One lane per path.  gain = (float)(1 + kappaMax * rho) with kappaMax the path's largest heading rate per metre.
__global__ void __launch_bounds__(kBlock) k_check_arcs_footprint(MapView m, Footprint fp, int64_t n, const double* __restrict__ from, const double* __restrict__ kappa,
	const double* __restrict__ length, const int32_t* __restrict__ dir, uint8_t* __restrict__ valid, float* __restrict__ last)
{
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
		Arc a;
		a.init = { from[3 * i], from[3 * i + 1], from[3 * i + 2] };
		a.kappa = kappa[i];
		a.length = length[i];
		a.backward = dir[i] == 1;
		float l = -1.0f;
		int checks = 0;
		const bool ok = is_path_valid_fp(m, fp, fp_gain(fp, fabs(a.kappa)), a, a.init, l, checks);
		valid[i] = ok ? 1 : 0;
		if (last)
			last[i] = l;
	}
}

__global__ void __launch_bounds__(kBlock) k_check_rs_paths_footprint(MapView m, Footprint fp, int64_t n, const pp_rs_path* __restrict__ paths, uint8_t* __restrict__ valid,
	float* __restrict__ last)
{
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
		const rs::Path p = load_path(paths[i]);
		float l = -1.0f;
		int checks = 0;
		const bool ok = is_path_valid_fp(m, fp, fp_gain(fp, 1.0 / p.rmin), p, p.init, l, checks); // every turning motion has |kappa| = 1 / rmin
		valid[i] = ok ? 1 : 0;
		if (last)
			last[i] = l;
	}
}

__global__ void __launch_bounds__(kBlock) k_check_se2_paths_footprint(MapView m, Footprint fp, int64_t n, const double* __restrict__ from, const double* __restrict__ to,
	uint8_t* __restrict__ valid, float* __restrict__ last)
{
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
		Se2Line p;
		p.init = { from[3 * i], from[3 * i + 1], wrap_theta(from[3 * i + 2]) };
		p.fin = { to[3 * i], to[3 * i + 1], wrap_theta(to[3 * i + 2]) };
		const double dx = p.fin.x - p.init.x, dy = p.fin.y - p.init.y;
		p.length = sqrt(dx * dx + dy * dy);
		// the heading is linear in the travelled length: |dtheta| / length radians per metre (a zero-length path never steps)
		const float gain = p.length == 0.0 ? 1.0f : fp_gain(fp, fabs(p.fin.t - p.init.t) / p.length);
		float l = -1.0f;
		int checks = 0;
		const bool ok = is_path_valid_fp(m, fp, gain, p, p.init, l, checks);
		valid[i] = ok ? 1 : 0;
		if (last)
			last[i] = l;
	}
}

int bad(const char* msg)
{
	set_error(msg);
	return PP_ERR_INVALID;
}

} // namespace

namespace pph {

int footprint_prepare(pp_map* map, pp_footprint* fp, bool needBits)
{
	if (!map || !fp)
		return bad("null map or footprint");
	if (fp->map != map)
		return bad("the footprint belongs to another map: create one for this map with pp_footprint_create");
	if (!map->dist)
		return bad("distance grid not uploaded (pp_map_upload_dist2 / pp_map_upload_distance / pp_map_update_gvd)");
	if (!needBits || (fp->bitsBuilt && fp->bitsVersion == map->distVersion))
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	const int64_t cells = (int64_t)map->cells();
	fp->wordsPer = (uint32_t)(((cells + 63) / 64) * 2); // whole 64-cell groups, as pp_map::validBits
	PP_HIP_TRY(fp->bits.ensure((size_t)fp->nRadii * fp->wordsPer * 4));
	for (int k = 0; k < fp->nRadii; k++)
		PP_HIP_TRY(launch_valid_bits(map->ctx->stream, map->dist, cells, fp->radii[k], fp->bits + (size_t)k * fp->wordsPer));
	fp->bitsBuilt = true;
	fp->bitsVersion = map->distVersion;
	return PP_OK;
}

hipError_t launch_check_states_footprint(hipStream_t s, const MapView& m, const pp_footprint* fp, int64_t n, const double* poses, uint8_t* valid, float* clearance)
{
	if (n <= 0)
		return hipSuccess;
	int64_t done = 0;
	constexpr int kTile = kBlock * kPer;
	const bool aligned = (((uintptr_t)poses) & 15) == 0 && (((uintptr_t)valid) & 3) == 0;
	if (!clearance && fp->bitsBuilt && aligned && n >= 64 * kTile) {
		const int64_t tiles = n / kTile;
		hipLaunchKernelGGL(k_check_states_footprint_pipe, dim3(grid_for(tiles, 1, 256 * 16)), dim3(kBlock), 0, s, m, fp->fp, fp->bits, fp->wordsPer, tiles,
			reinterpret_cast<const dvec2*>(poses), reinterpret_cast<uint32_t*>(valid));
		done = tiles * kTile;
	}
	if (done < n)
		hipLaunchKernelGGL(k_check_states_footprint, dim3(grid_for(n - done, kBlock)), dim3(kBlock), 0, s, m, fp->fp, n - done, poses + 3 * done, valid + done,
			clearance ? clearance + done : nullptr);
	return hipGetLastError();
}

} // namespace pph

extern "C" {

int pp_footprint_cover_rectangle(double length, double width, double rear_overhang, int32_t n_discs, pp_footprint_disc* discs_out)
{
	if (!discs_out)
		return bad("null discs_out");
	if (n_discs < 1 || n_discs > PP_FOOTPRINT_MAX_DISCS)
		return bad("a footprint has 1 to 8 discs (PP_FOOTPRINT_MAX_DISCS)");
	if (!(length > 0.0) || !(width > 0.0) || !std::isfinite(length) || !std::isfinite(width) || !std::isfinite(rear_overhang))
		return bad("length and width must be positive and finite, rear_overhang finite");
	const double s = length / n_discs;
	const double rd = std::sqrt((s / 2) * (s / 2) + (width / 2) * (width / 2));
	float r = (float)rd;
	if ((double)r < rd)
		r = std::nextafterf(r, INFINITY); // rounded up: the float discs still cover the rectangle
	for (int i = 0; i < n_discs; i++) {
		discs_out[i].ox = -rear_overhang + (i + 0.5) * s;
		discs_out[i].oy = 0.0;
		discs_out[i].r = r;
		discs_out[i].pad = 0.0f;
	}
	return PP_OK;
}

int pp_footprint_create(pp_map* map, int32_t n_discs, const pp_footprint_disc* discs, pp_footprint** out)
{
	if (!map || !discs || !out)
		return bad("null argument");
	if (n_discs < 1 || n_discs > PP_FOOTPRINT_MAX_DISCS)
		return bad("a footprint has 1 to 8 discs (PP_FOOTPRINT_MAX_DISCS): cover the vehicle with fewer, larger discs");
	auto f = std::make_unique<pp_footprint>();
	f->fp.n = n_discs;
	f->fp.anyOffset = 0;
	f->fp.rho = 0.0;
	for (int i = 0; i < kFootprintMaxDiscs; i++) {
		f->fp.ox[i] = f->fp.oy[i] = 0.0;
		f->fp.r[i] = 0.0f;
		f->fp.slot[i] = 0;
	}
	for (int i = 0; i < n_discs; i++) {
		const pp_footprint_disc& d = discs[i];
		if (!std::isfinite(d.ox) || !std::isfinite(d.oy) || !std::isfinite(d.r) || d.r < 0.0f)
			return bad("footprint disc centres must be finite and radii finite and >= 0");
		f->fp.ox[i] = d.ox;
		f->fp.oy[i] = d.oy;
		f->fp.r[i] = d.r;
		if (d.ox != 0.0 || d.oy != 0.0)
			f->fp.anyOffset = 1;
		f->fp.rho = std::fmax(f->fp.rho, std::hypot(d.ox, d.oy));
		int slot = -1;
		for (int k = 0; k < f->nRadii; k++)
			if (f->radii[k] == d.r)
				slot = k;
		if (slot < 0) {
			slot = f->nRadii++;
			f->radii[slot] = d.r;
		}
		f->fp.slot[i] = slot;
	}
	f->map = map;
	__atomic_add_fetch(&map->refs, 1, __ATOMIC_RELAXED); // the footprint keeps its map alive
	*out = f.release();
	return PP_OK;
}

int pp_footprint_destroy(pp_footprint* fp)
{
	pph::footprint_release(fp);
	return PP_OK;
}

int pp_check_states_footprint_dev(pp_map* map, pp_footprint* fp, int64_t n, const double* poses_dev, uint8_t* valid_dev)
{
	if (n < 0 || (n > 0 && (!poses_dev || !valid_dev)))
		return bad("invalid arguments");
	if (int rc = pph::footprint_prepare(map, fp, true))
		return rc;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	PP_HIP_TRY(pph::launch_check_states_footprint(map->ctx->stream, map->view(), fp, n, poses_dev, valid_dev, nullptr));
	return PP_OK;
}

int pp_check_states_footprint(pp_map* map, pp_footprint* fp, int64_t n, const double* poses_host, uint8_t* valid_host, float* clearance_host)
{
	if (n < 0 || (n > 0 && (!poses_host || !valid_host)))
		return bad("invalid arguments");
	if (int rc = pph::footprint_prepare(map, fp, clearance_host == nullptr))
		return rc;
	if (n == 0)
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	hipStream_t s = map->ctx->stream;
	pph::DeviceMem dp, dv, dc;
	PP_HIP_TRY(dp.alloc((size_t)n * 24));
	PP_HIP_TRY(dv.alloc((size_t)n));
	if (clearance_host)
		PP_HIP_TRY(dc.alloc((size_t)n * 4));
	PP_HIP_TRY(hipMemcpyAsync(dp.get(), poses_host, (size_t)n * 24, hipMemcpyHostToDevice, s));
	PP_HIP_TRY(pph::launch_check_states_footprint(s, map->view(), fp, n, dp.as<double>(), dv.as<uint8_t>(), dc.as<float>()));
	PP_HIP_TRY(hipMemcpyAsync(valid_host, dv.get(), (size_t)n, hipMemcpyDeviceToHost, s));
	if (clearance_host)
		PP_HIP_TRY(hipMemcpyAsync(clearance_host, dc.get(), (size_t)n * 4, hipMemcpyDeviceToHost, s));
	PP_HIP_TRY(hipStreamSynchronize(s));
	return PP_OK;
}

int pp_check_arcs_footprint_dev(pp_map* map, pp_footprint* fp, int64_t n, const double* from_dev, const double* curvature_dev, const double* length_dev,
	const int32_t* direction_dev, uint8_t* valid_dev, float* last_ratio_dev)
{
	if (n < 0 || (n > 0 && (!from_dev || !curvature_dev || !length_dev || !direction_dev || !valid_dev)))
		return bad("invalid arguments");
	if (int rc = pph::footprint_prepare(map, fp, false))
		return rc;
	if (n == 0)
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	hipLaunchKernelGGL(k_check_arcs_footprint, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, map->ctx->stream, map->view(), fp->fp, n, from_dev, curvature_dev, length_dev,
		direction_dev, valid_dev, last_ratio_dev);
	PP_HIP_TRY(hipGetLastError());
	return PP_OK;
}

int pp_check_arcs_footprint(pp_map* map, pp_footprint* fp, int64_t n, const double* from_host, const double* curvature_host, const double* length_host,
	const int32_t* direction_host, uint8_t* valid_host, float* last_ratio_host)
{
	if (n < 0 || (n > 0 && (!from_host || !curvature_host || !length_host || !direction_host || !valid_host)))
		return bad("invalid arguments");
	if (int rc = pph::footprint_prepare(map, fp, false))
		return rc;
	if (n == 0)
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	hipStream_t s = map->ctx->stream;
	pph::DeviceMem df, dk, dl, dd, dv, dr;
	PP_HIP_TRY(df.alloc((size_t)n * 24));
	PP_HIP_TRY(dk.alloc((size_t)n * 8));
	PP_HIP_TRY(dl.alloc((size_t)n * 8));
	PP_HIP_TRY(dd.alloc((size_t)n * 4));
	PP_HIP_TRY(dv.alloc((size_t)n));
	PP_HIP_TRY(dr.alloc((size_t)n * 4));
	PP_HIP_TRY(hipMemcpyAsync(df.get(), from_host, (size_t)n * 24, hipMemcpyHostToDevice, s));
	PP_HIP_TRY(hipMemcpyAsync(dk.get(), curvature_host, (size_t)n * 8, hipMemcpyHostToDevice, s));
	PP_HIP_TRY(hipMemcpyAsync(dl.get(), length_host, (size_t)n * 8, hipMemcpyHostToDevice, s));
	PP_HIP_TRY(hipMemcpyAsync(dd.get(), direction_host, (size_t)n * 4, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(k_check_arcs_footprint, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, map->view(), fp->fp, n, df.as<double>(), dk.as<double>(), dl.as<double>(),
		dd.as<int32_t>(), dv.as<uint8_t>(), dr.as<float>());
	PP_HIP_TRY(hipGetLastError());
	PP_HIP_TRY(hipMemcpyAsync(valid_host, dv.get(), (size_t)n, hipMemcpyDeviceToHost, s));
	if (last_ratio_host)
		PP_HIP_TRY(hipMemcpyAsync(last_ratio_host, dr.get(), (size_t)n * 4, hipMemcpyDeviceToHost, s));
	PP_HIP_TRY(hipStreamSynchronize(s));
	return PP_OK;
}

int pp_check_rs_paths_footprint_dev(pp_map* map, pp_footprint* fp, int64_t n, const pp_rs_path* paths_dev, uint8_t* valid_dev, float* last_ratio_dev)
{
	if (n < 0 || (n > 0 && (!paths_dev || !valid_dev)))
		return bad("invalid arguments");
	if (int rc = pph::footprint_prepare(map, fp, false))
		return rc;
	if (n == 0)
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	hipLaunchKernelGGL(k_check_rs_paths_footprint, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, map->ctx->stream, map->view(), fp->fp, n, paths_dev, valid_dev, last_ratio_dev);
	PP_HIP_TRY(hipGetLastError());
	return PP_OK;
}

int pp_check_rs_paths_footprint(pp_map* map, pp_footprint* fp, int64_t n, const pp_rs_path* paths_host, uint8_t* valid_host, float* last_ratio_host)
{
	if (n < 0 || (n > 0 && (!paths_host || !valid_host)))
		return bad("invalid arguments");
	if (int rc = pph::footprint_prepare(map, fp, false))
		return rc;
	if (n == 0)
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	hipStream_t s = map->ctx->stream;
	pph::DeviceMem dp, dv, dl;
	PP_HIP_TRY(dp.alloc((size_t)n * sizeof(pp_rs_path)));
	PP_HIP_TRY(dv.alloc((size_t)n));
	PP_HIP_TRY(dl.alloc((size_t)n * 4));
	PP_HIP_TRY(hipMemcpyAsync(dp.get(), paths_host, (size_t)n * sizeof(pp_rs_path), hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(k_check_rs_paths_footprint, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, map->view(), fp->fp, n, dp.as<pp_rs_path>(), dv.as<uint8_t>(), dl.as<float>());
	PP_HIP_TRY(hipGetLastError());
	PP_HIP_TRY(hipMemcpyAsync(valid_host, dv.get(), (size_t)n, hipMemcpyDeviceToHost, s));
	if (last_ratio_host)
		PP_HIP_TRY(hipMemcpyAsync(last_ratio_host, dl.get(), (size_t)n * 4, hipMemcpyDeviceToHost, s));
	PP_HIP_TRY(hipStreamSynchronize(s));
	return PP_OK;
}

int pp_check_se2_paths_footprint(pp_map* map, pp_footprint* fp, int64_t n, const double* from_host, const double* to_host, uint8_t* valid_host, float* last_ratio_host)
{
	if (n < 0 || (n > 0 && (!from_host || !to_host || !valid_host)))
		return bad("invalid arguments");
	if (int rc = pph::footprint_prepare(map, fp, false))
		return rc;
	if (n == 0)
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	hipStream_t s = map->ctx->stream;
	pph::DeviceMem df, dt, dv, dl;
	PP_HIP_TRY(df.alloc((size_t)n * 24));
	PP_HIP_TRY(dt.alloc((size_t)n * 24));
	PP_HIP_TRY(dv.alloc((size_t)n));
	PP_HIP_TRY(dl.alloc((size_t)n * 4));
	PP_HIP_TRY(hipMemcpyAsync(df.get(), from_host, (size_t)n * 24, hipMemcpyHostToDevice, s));
	PP_HIP_TRY(hipMemcpyAsync(dt.get(), to_host, (size_t)n * 24, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(k_check_se2_paths_footprint, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, map->view(), fp->fp, n, df.as<double>(), dt.as<double>(), dv.as<uint8_t>(),
		dl.as<float>());
	PP_HIP_TRY(hipGetLastError());
	PP_HIP_TRY(hipMemcpyAsync(valid_host, dv.get(), (size_t)n, hipMemcpyDeviceToHost, s));
	if (last_ratio_host)
		PP_HIP_TRY(hipMemcpyAsync(last_ratio_host, dl.get(), (size_t)n * 4, hipMemcpyDeviceToHost, s));
	PP_HIP_TRY(hipStreamSynchronize(s));
	return PP_OK;
}

} // extern "C"

namespace pph {
void footprint_release(pp_footprint* fp)
{
	if (!fp || __atomic_sub_fetch(&fp->refs, 1, __ATOMIC_ACQ_REL) > 0)
		return;
	pp_map* map = fp->map;
	if (fp->bits) {
		(void)hipSetDevice(map->ctx->device);
		(void)hipStreamSynchronize(map->ctx->stream);
	}
	delete fp;
	map_release(map);
}
} // namespace pph
