// pybind11 module `pyplanning`: the reference's Python surface (interfaces/python/src/pyplanning.cpp), same class / method names, backed
// by libpphip.so through planner_hip.hpp.  Every name the reference's module binds is bound here (tests/golden/pyplanning_bound_names.json,
// tests/test_pyplanning_surface.py): initialize, Status, Point2d, Pose2d, GridCellPosition, Steer, Direction, the path value types and
// connections, KinematicBicycleModel, StateSpaceSE2, OccupancyMap (+ set_grids), ObstacleListOccupancyMap, Obstacle and the shapes, GVD,
// StateValidatorSE2Base / SE2Free / OccupancyMap, HybridAStarSearchParameters / SmootherParameters / Stats, PathPlannerSE2Base, HybridAStar,
// the N2 heuristics / propagators / planners.  New surface next to it: search_batch, GridAStarBatch, RRT / RRTStar (the reference does not
// bind RRT).
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/operators.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "planner_hip.hpp"
#include "a_star.hpp"
#include "map_authoring.hpp"

namespace py = pybind11;
using namespace Planner;

PYBIND11_MODULE(pyplanning, m)
{
	m.def("initialize", []() {}); // PP_INIT: logging / profiler singletons of the reference; nothing to set up here

	py::enum_<Status>(m, "Status").value("SUCCESS", Status::Success).value("FAILURE", Status::Failure);
	py::enum_<Steer>(m, "Steer").value("LEFT", Steer::Left).value("STRAIGHT", Steer::Straight).value("RIGHT", Steer::Right);
	py::enum_<Direction>(m, "Direction").value("FORWARD", Direction::Forward).value("BACKWARD", Direction::Backward).value("NO_MOTION", Direction::NoMotion);

	py::class_<Point2d>(m, "Point2d")
		.def(py::init<double, double>())
		.def("x", [](Point2d& p) { return p.x(); })
		.def("y", [](Point2d& p) { return p.y(); })
		.def(py::self + py::self)
		.def(py::self - py::self)
		.def(py::self == py::self)
		.def(py::self != py::self);

	py::class_<Pose2d>(m, "Pose2d")
		.def(py::init<const Point2d&, double>())
		.def(py::init<double, double, double>())
		.def_readwrite("position", &Pose2d::position)
		.def_readwrite("theta", &Pose2d::theta)
		.def("x", [](Pose2d& p) { return p.x(); })
		.def("y", [](Pose2d& p) { return p.y(); })
		.def(py::self + py::self)
		.def(py::self - py::self)
		.def(py::self == py::self)
		.def(py::self != py::self);

	// ---- paths (pyplanning.cpp:247-309) ----
	struct PathSE2BaseWrapper : PathSE2Base {
		using PathSE2Base::PathSE2Base;
		Pose2d Interpolate(double ratio) const override { PYBIND11_OVERRIDE_PURE(Pose2d, PathSE2Base, Interpolate, ratio); }
		void Truncate(double ratio) override { PYBIND11_OVERRIDE_PURE(void, PathSE2Base, Truncate, ratio); }
	};
	py::class_<PathSE2Base, Ref<PathSE2Base>, PathSE2BaseWrapper>(m, "PathSE2Base")
		.def(py::init<>())
		.def(py::init<Pose2d, double>(), py::arg("init"), py::arg("length") = 0.0)
		.def("get_initial_state", &PathSE2Base::GetInitialState)
		.def("get_final_state", &PathSE2Base::GetFinalState)
		.def("interpolate", py::overload_cast<double>(&PathSE2Base::Interpolate, py::const_))
		.def("interpolate", py::overload_cast<const std::vector<double>&>(&PathSE2Base::Interpolate, py::const_))
		.def("truncate", &PathSE2Base::Truncate)
		.def("get_length", &PathSE2Base::GetLength);
	py::class_<PathSE2, Ref<PathSE2>, PathSE2Base>(m, "PathSE2").def(py::init<const Pose2d&, const Pose2d&>());
	py::class_<PathNonHolonomicSE2Base, Ref<PathNonHolonomicSE2Base>, PathSE2Base>(m, "PathNonHolonomicSE2Base")
		.def("get_direction", &PathNonHolonomicSE2Base::GetDirection)
		.def("get_cusp_point_ratios", &PathNonHolonomicSE2Base::GetCuspPointRatios);
	py::class_<PathReedsShepp, Ref<PathReedsShepp>, PathNonHolonomicSE2Base>(m, "PathReedsShepp")
		.def("interpolate", py::overload_cast<double>(&PathReedsShepp::Interpolate, py::const_))
		.def("interpolate", py::overload_cast<const std::vector<double>&>(&PathReedsShepp::Interpolate, py::const_))
		.def_property("min_turning_radius", &PathReedsShepp::GetMinTurningRadius, nullptr)
		.def_property_readonly("word", [](const PathReedsShepp& p) { return p.Record().word; })
		.def_property_readonly("motions", [](const PathReedsShepp& p) {
			py::list out;
			const pp_rs_path& r = p.Record();
			for (int i = 0; i < 5; i++)
				if (r.motion_length[i] != INFINITY && r.direction[i] != 2)
					out.append(py::make_tuple((Steer)r.steer[i], (Direction)r.direction[i], r.motion_length[i]));
				else
					break;
			return out;
		});
	py::class_<KinematicBicycleModel, Ref<KinematicBicycleModel>>(m, "KinematicBicycleModel")
		.def(py::init<double, double>(), py::arg("wheelbase") = 2.6, py::arg("rear_to_center") = 0.0)
		.def("constant_steer", &KinematicBicycleModel::ConstantSteer, py::arg("from"), py::arg("steering"), py::arg("dist"), py::arg("direction") = Direction::Forward)
		.def("get_steering_angle_from_turning_radius", &KinematicBicycleModel::GetSteeringAngleFromTurningRadius);
	py::class_<PathConstantSteer, Ref<PathConstantSteer>, PathNonHolonomicSE2Base>(m, "PathConstantSteer")
		.def(py::init<const Ref<KinematicBicycleModel>&, const Pose2d&, double, double, Direction>())
		.def_property("steering", &PathConstantSteer::GetSteeringAngle, nullptr);
	struct PathConnectionSE2BaseWrapper : PathConnectionSE2Base {
		using PathConnectionSE2Base::PathConnectionSE2Base;
		Ref<PathSE2Base> Connect(const Pose2d& from, const Pose2d& to) override { PYBIND11_OVERRIDE_PURE(Ref<PathSE2Base>, PathConnectionSE2Base, Connect, from, to); }
	};
	py::class_<PathConnectionSE2Base, Ref<PathConnectionSE2Base>, PathConnectionSE2BaseWrapper>(m, "PathConnectionSE2Base")
		.def(py::init<>())
		.def("connect", &PathConnectionSE2Base::Connect);
	py::class_<PathConnectionSE2, Ref<PathConnectionSE2>, PathConnectionSE2Base>(m, "PathConnectionSE2").def(py::init<>());
	py::class_<PathConnectionReedsShepp, Ref<PathConnectionReedsShepp>, PathConnectionSE2Base>(m, "PathConnectionReedsShepp")
		.def(py::init<double, double, double, double>(), py::arg("min_turning_radius") = 1.0, py::arg("direction_switching_cost") = 0.0, py::arg("reverse_cost_multiplier") = 1.0,
			py::arg("forward_cost_multiplier") = 1.0);

	py::class_<GridCellPosition>(m, "GridCellPosition")
		.def(py::init<>())
		.def(py::init<int, int>())
		.def_readwrite("row", &GridCellPosition::row)
		.def_readwrite("col", &GridCellPosition::col)
		.def(py::self == py::self)
		.def(py::self != py::self)
		.def("__hash__", [](const GridCellPosition& c) { return std::hash<GridCellPosition>()(c); })
		.def("__repr__", [](const GridCellPosition& c) { return "<GridCellPosition: row " + std::to_string(c.row) + ", col: " + std::to_string(c.col) + ">"; });

	py::class_<StateSpaceSE2, Ref<StateSpaceSE2>>(m, "StateSpaceSE2")
		.def(py::init<const std::array<Pose2d, 2>&>())
		.def(py::init<const Pose2d&, const Pose2d&>())
		.def("enforce_bounds", &StateSpaceSE2::EnforceBounds)
		.def("validate_bounds", &StateSpaceSE2::ValidateBounds)
		.def("sample_uniform", &StateSpaceSE2::SampleUniform)   // pyplanning.cpp:325
		.def("sample_gaussian", &StateSpaceSE2::SampleGaussian) // pyplanning.cpp:326
		.def_readonly("bounds", &StateSpaceSE2::bounds);
	// not in the reference (its engine is seeded from std::random_device only): a fixed seed for the global engine the two samplers draw from
	m.def("seed_random", [](unsigned long long seed) { Random<double>::Seed(seed); });

	struct OccupancyMapWrapper : OccupancyMap { // pyplanning.cpp:337-341: Python may subclass the map
		using OccupancyMap::OccupancyMap;
		bool IsOccupied(const GridCellPosition& a) override { PYBIND11_OVERRIDE(bool, OccupancyMap, IsOccupied, a); }
	};
	py::class_<OccupancyMap, Ref<OccupancyMap>, OccupancyMapWrapper>(m, "OccupancyMap")
		.def(py::init<float>())
		.def("initialize_size", &OccupancyMap::InitializeSize)
		.def("rows", &OccupancyMap::Rows)
		.def("columns", &OccupancyMap::Columns)
		.def("set_position", &OccupancyMap::SetPosition)
		.def("get_position", &OccupancyMap::GetPosition)
		.def("update", &OccupancyMap::Update)
		.def("is_occupied", &OccupancyMap::IsOccupied)
		.def("is_occupied)", &OccupancyMap::IsOccupied) // the name the reference actually registers (pyplanning.cpp:351, a typo): reachable by getattr only
		// bound by the reference (pyplanning.cpp:354) although GVD::ObstacleDistanceMap is not a bound class: calling it there raises
		// TypeError ("Unable to convert function return value to a Python type"); the same here
		.def("get_obstacle_map", [](OccupancyMap&) -> py::object {
			throw py::type_error("Unable to convert function return value to a Python type! The signature was\n\t(self: pyplanning.OccupancyMap) -> GVD::ObstacleDistanceMap");
		})
		.def("get_occupancy_value", py::overload_cast<int, int>(&OccupancyMap::GetOccupancyValue))
		.def("get_occupancy_value", py::overload_cast<const GridCellPosition&>(&OccupancyMap::GetOccupancyValue))
		.def("grid_cell_to_local_position", &OccupancyMap::GridCellToLocalPosition)
		.def("local_position_to_grid_cell", &OccupancyMap::LocalPositionToGridCell, py::arg("position"), py::arg("bounded") = true)
		.def("local_position_to_world_position", &OccupancyMap::LocalPositionToWorldPosition)
		.def("world_position_to_local_position", &OccupancyMap::WorldPositionToLocalPosition)
		.def("occupancy", [](OccupancyMap& map) {
			py::array_t<int32_t> a({ map.Rows(), map.Columns() });
			std::copy(map.Occupancy().begin(), map.Occupancy().end(), a.mutable_data());
			return a;
		})
		.def("world_position_to_grid_cell", &OccupancyMap::WorldPositionToGridCell, py::arg("position"), py::arg("bounded") = true)
		.def("grid_cell_to_world_position", &OccupancyMap::GridCellToWorldPosition)
		.def("is_inside_map", py::overload_cast<const GridCellPosition&>(&OccupancyMap::IsInsideMap, py::const_))
		.def("is_inside_map", py::overload_cast<const Point2d&>(&OccupancyMap::IsInsideMap, py::const_))
		.def("set_grids",
			[](OccupancyMap& map, py::array_t<int32_t, py::array::c_style | py::array::forcecast> occ, py::array_t<int32_t, py::array::c_style | py::array::forcecast> d2,
				py::array_t<float, py::array::c_style | py::array::forcecast> pc) {
				const size_t n = (size_t)map.Rows() * map.Columns();
				if ((size_t)occ.size() != n || (size_t)d2.size() != n || (size_t)pc.size() != n)
					throw std::invalid_argument("set_grids: arrays must be rows x columns");
				map.SetGrids(occ.data(), d2.data(), pc.data());
			},
			py::arg("occupancy"), py::arg("dist2"), py::arg("path_cost"))
		.def("set_distances",
			[](OccupancyMap& map, py::array_t<float, py::array::c_style | py::array::forcecast> d) {
				if ((size_t)d.size() != (size_t)map.Rows() * map.Columns())
					throw std::invalid_argument("set_distances: array must be rows x columns");
				map.SetDistances(d.data());
			},
			py::arg("distance"))
		.def("get_distance_to_nearest_obstacle", &OccupancyMap::GetDistanceToNearestObstacle)
		.def("set_nearest_cells",
			[](OccupancyMap& map, py::array_t<int32_t, py::array::c_style | py::array::forcecast> o, py::array_t<int32_t, py::array::c_style | py::array::forcecast> e) {
				const size_t n = (size_t)map.Rows() * map.Columns() * 2;
				if ((size_t)o.size() != n || (size_t)e.size() != n)
					throw std::invalid_argument("set_nearest_cells: arrays must be rows x columns x 2");
				map.SetNearestCells(o.data(), e.data());
			},
			py::arg("nearest_obstacle"), py::arg("nearest_edge"));

	struct StateValidatorSE2BaseWrapper : StateValidatorSE2Base { // pyplanning.cpp:402-406 (whose IsPathValid trampoline dispatches to IsStateValid, Q18)
		using StateValidatorSE2Base::StateValidatorSE2Base;
		bool IsStateValid(const Pose2d& a) override { PYBIND11_OVERRIDE_PURE(bool, StateValidatorSE2Base, IsStateValid, a); }
		bool IsPathValid(const PathSE2Base& a, float* b) override { PYBIND11_OVERRIDE_PURE(bool, StateValidatorSE2Base, IsPathValid, a, b); }
	};
	py::class_<StateValidatorSE2Base, Ref<StateValidatorSE2Base>, StateValidatorSE2BaseWrapper>(m, "StateValidatorSE2Base")
		.def(py::init<const Ref<StateSpaceSE2>&>())
		.def("is_state_valid", &StateValidatorSE2Base::IsStateValid)
		.def("is_path_valid", [](StateValidatorSE2Base& v, const PathSE2Base& path) { return v.IsPathValid(path, (float*)nullptr); })
		.def("is_path_valid_with_ratio",
			[](StateValidatorSE2Base& v, const PathSE2Base& path) {
				float last = 0.0f;
				const bool ok = v.IsPathValid(path, &last);
				return py::make_tuple(ok, last);
			})
		.def_property("state_space", &StateValidatorSE2Base::GetStateSpace, nullptr);
	py::class_<StateValidatorSE2Free, Ref<StateValidatorSE2Free>, StateValidatorSE2Base>(m, "StateValidatorSE2Free").def(py::init<const Ref<StateSpaceSE2>&>());

	// ---- map authoring (pyplanning.cpp:364-400, 423-435) ----
	py::class_<ObstacleListOccupancyMap, Ref<ObstacleListOccupancyMap>, OccupancyMap>(m, "ObstacleListOccupancyMap")
		.def(py::init<float>())
		.def("add_obstacle", &ObstacleListOccupancyMap::AddObstacle)
		.def("remove_obstacle", &ObstacleListOccupancyMap::RemoveObstacle)
		.def("get_num_obstacles", &ObstacleListOccupancyMap::GetNumObstacles);
	py::class_<Obstacle, Ref<Obstacle>>(m, "Obstacle")
		.def(py::init<>())
		.def("set_shape", &Obstacle::SetShape)
		.def("set_pose", &Obstacle::SetPose)
		.def("get_boundary_grid_cell_position", &Obstacle::GetBoundaryGridCellPosition)
		.def("get_boundary_world_position", &Obstacle::GetBoundaryWorldPosition);
	struct ShapeWrapper : Shape {
		using Shape::Shape;
		void GetGridCellsPosition(OccupancyMap& a, const Pose2d& b, std::vector<GridCellPosition>& c) override { PYBIND11_OVERRIDE_PURE(void, Shape, GetGridCellsPosition, a, b, c); }
		void GetVerticesPosition(const Pose2d& a, std::vector<Point2d>& b) override { PYBIND11_OVERRIDE_PURE(void, Shape, GetVerticesPosition, a, b); }
	};
	py::class_<Shape, Ref<Shape>, ShapeWrapper>(m, "Shape").def(py::init<>());
	py::class_<CompositeShape, Ref<CompositeShape>, Shape>(m, "CompositeShape").def(py::init<>()).def("add", &CompositeShape::Add);
	py::class_<PolygonShape, Ref<PolygonShape>, Shape>(m, "PolygonShape").def(py::init<const std::vector<Point2d>&>());
	py::class_<RegularPolygonShape, Ref<RegularPolygonShape>, Shape>(m, "RegularPolygonShape").def(py::init<double, int>());
	py::class_<RectangleShape, Ref<RectangleShape>, Shape>(m, "RectangleShape").def(py::init<double, double>());
	py::class_<CircleShape, Ref<CircleShape>, Shape>(m, "CircleShape").def(py::init<double, int>());
	py::class_<GVD>(m, "GVD")
		.def(py::init<const Ref<OccupancyMap>&>())
		.def("update", &GVD::Update)
		// not in the reference's module: how Update builds the two distance maps ("reference_order", the default: the reference's
		// brushfire bit for bit; "exact_transform": the device's exact Euclidean transform, see pp_hip.h: pp_map_update_gvd_ex)
		.def("set_update_mode", [](GVD& g, const std::string& mode) {
			if (mode == "reference_order")
				g.SetUpdateMode(OccupancyMap::FieldUpdateMode::ReferenceOrder);
			else if (mode == "exact_transform")
				g.SetUpdateMode(OccupancyMap::FieldUpdateMode::ExactTransform);
			else
				throw std::invalid_argument("mode: 'reference_order' or 'exact_transform'");
		})
		.def("get_distance_to_nearest_obstacle", py::overload_cast<int, int>(&GVD::GetDistanceToNearestObstacle, py::const_))
		.def("get_distance_to_nearest_obstacle", py::overload_cast<const GridCellPosition&>(&GVD::GetDistanceToNearestObstacle, py::const_))
		.def("get_distance_to_nearest_voronoi_edge", py::overload_cast<int, int>(&GVD::GetDistanceToNearestVoronoiEdge, py::const_))
		.def("get_distance_to_nearest_voronoi_edge", py::overload_cast<const GridCellPosition&>(&GVD::GetDistanceToNearestVoronoiEdge, py::const_))
		.def("get_path_cost", py::overload_cast<int, int>(&GVD::GetPathCost, py::const_))
		.def("get_path_cost", py::overload_cast<const GridCellPosition&>(&GVD::GetPathCost, py::const_))
		.def("get_nearest_obstacle_cell", py::overload_cast<int, int>(&GVD::GetNearestObstacleCell, py::const_))
		.def("get_nearest_voronoi_edge_cell", py::overload_cast<int, int>(&GVD::GetNearestVoronoiEdgeCell, py::const_))
		.def("visualize", &GVD::Visualize);

	py::class_<StateValidatorOccupancyMap, Ref<StateValidatorOccupancyMap>, StateValidatorSE2Base>(m, "StateValidatorOccupancyMap")
		.def(py::init<const Ref<StateSpaceSE2>&, const Ref<OccupancyMap>&>())
		.def("get_occupancy_map", &StateValidatorOccupancyMap::GetOccupancyMap)
		.def("is_state_valid", py::overload_cast<const Pose2d&>(&StateValidatorOccupancyMap::IsStateValid))
		.def("is_states_valid",
			[](StateValidatorOccupancyMap& v, py::array_t<double, py::array::c_style | py::array::forcecast> poses) {
				if (poses.ndim() != 2 || poses.shape(1) != 3)
					throw std::invalid_argument("poses must be (n, 3)");
				py::array_t<uint8_t> out(poses.shape(0));
				if (poses.shape(0))
				{
					pp_map* dev = v.Device();
					if (pp_footprint* fp = v.DeviceFootprint())
						ppCheck(pp_check_states_footprint(dev, fp, poses.shape(0), poses.data(), out.mutable_data(), nullptr));
					else
						ppCheck(pp_check_states(dev, poses.shape(0), poses.data(), out.mutable_data()));
				}
				return out;
			})
		.def("is_arc_valid",
			[](StateValidatorOccupancyMap& v, const Pose2d& from, double curvature, double length, Direction dir) {
				float last = 0;
				bool ok = v.IsArcValid(from, curvature, length, dir, &last);
				return py::make_tuple(ok, last);
			})
		// vehicle footprint (include/pp_hip.h): discs (ox, oy, r) in the vehicle frame instead of the reference point against min_safe_radius
		.def("set_footprint",
			[](StateValidatorOccupancyMap& v, const std::vector<std::tuple<double, double, double>>& discs) {
				std::vector<FootprintDisc> d;
				for (const auto& t : discs)
					d.push_back({ std::get<0>(t), std::get<1>(t), (float)std::get<2>(t) });
				v.SetFootprint(d);
				v.Device();
				v.DeviceFootprint(); // bad values are refused here, not at the first check
			})
		.def("clear_footprint", &StateValidatorOccupancyMap::ClearFootprint)
		.def_property_readonly("footprint",
			[](const StateValidatorOccupancyMap& v) {
				std::vector<std::tuple<double, double, double>> out;
				for (const auto& d : v.GetFootprint())
					out.emplace_back(d.ox, d.oy, (double)d.r);
				return out;
			})
		.def_readwrite("min_path_interpolation_distance", &StateValidatorOccupancyMap::minPathInterpolationDistance)
		.def_readwrite("min_safe_radius", &StateValidatorOccupancyMap::minSafeRadius);
	m.def("rectangle_footprint", [](double length, double width, double rear_overhang, int n_discs) {
		std::vector<std::tuple<double, double, double>> out;
		for (const auto& d : RectangleFootprint(length, width, rear_overhang, n_discs))
			out.emplace_back(d.ox, d.oy, (double)d.r);
		return out;
	}, py::arg("length"), py::arg("width"), py::arg("rear_overhang"), py::arg("n_discs"));

	struct PathPlannerSE2BaseWrapper : PathPlannerSE2Base {
		using PathPlannerSE2Base::PathPlannerSE2Base;
		Status SearchPath() override { PYBIND11_OVERRIDE_PURE(Status, PathPlannerSE2Base, SearchPath); }
		std::vector<Pose2d> GetPath() const override { PYBIND11_OVERRIDE_PURE(std::vector<Pose2d>, PathPlannerSE2Base, GetPath); }
	};
	py::class_<PathPlannerSE2Base, PathPlannerSE2BaseWrapper>(m, "PathPlannerSE2Base")
		.def(py::init<>())
		.def("search_path", &PathPlannerSE2Base::SearchPath)
		.def("get_path", &PathPlannerSE2Base::GetPath)
		.def("set_init_state", &PathPlannerSE2Base::SetInitState)
		.def("set_goal_state", &PathPlannerSE2Base::SetGoalState);

	py::class_<HybridAStar::SearchParameters>(m, "HybridAStarSearchParameters")
		.def(py::init<>())
		.def(py::init<double, double, double, double, double, unsigned int, double, double>())
		.def_readonly("wheelbase", &HybridAStar::SearchParameters::wheelbase)
		.def_readonly("min_turning_radius", &HybridAStar::SearchParameters::minTurningRadius)
		.def_readonly("direction_switching_cost", &HybridAStar::SearchParameters::directionSwitchingCost)
		.def_readonly("reverse_cost_multiplier", &HybridAStar::SearchParameters::reverseCostMultiplier)
		.def_readonly("forward_cost_multiplier", &HybridAStar::SearchParameters::forwardCostMultiplier)
		.def_readonly("voronoi_cost_multiplier", &HybridAStar::SearchParameters::voronoiCostMultiplier)
		.def_readonly("num_generated_motion", &HybridAStar::SearchParameters::numGeneratedMotion)
		.def_readonly("spatial_resolution", &HybridAStar::SearchParameters::spatialResolution)
		.def_readonly("angular_resolution", &HybridAStar::SearchParameters::angularResolution);

	py::class_<Smoother::Parameters>(m, "HybridAStarSmootherParameters") // pyplanning.cpp:86-97
		.def(py::init<float>())
		.def_readwrite("step_tolerance", &Smoother::Parameters::stepTolerance)
		.def_readwrite("max_iterations", &Smoother::Parameters::maxIterations)
		.def_readwrite("learning_rate", &Smoother::Parameters::learningRate)
		.def_readwrite("path_weight", &Smoother::Parameters::pathWeight)
		.def_readwrite("smooth_weight", &Smoother::Parameters::smoothWeight)
		.def_readwrite("voronoi_weight", &Smoother::Parameters::voronoiWeight)
		.def_readwrite("collision_weight", &Smoother::Parameters::collisionWeight)
		.def_readwrite("curvature_weight", &Smoother::Parameters::curvatureWeight)
		.def_readwrite("collision_ratio", &Smoother::Parameters::collisionRatio)
		.def_readonly("max_curvature", &Smoother::Parameters::maxCurvature);
	py::enum_<Smoother::Status>(m, "SmoothingStatus") // pyplanning.cpp:103-108
		.value("MAX_ITERATION", Smoother::Status::MaxIteration)
		.value("STEP_TOLERANCE", Smoother::Status::StepTolerance)
		.value("PATH_SIZE", Smoother::Status::PathSize)
		.value("FAILURE", Smoother::Status::Failure)
		.value("COLLISION", Smoother::Status::Collision);
	py::class_<HybridAStar::Stats>(m, "HybridAStarStats")
		.def_readonly("graph_search_status", &HybridAStar::Stats::graphSearchStatus)
		.def_readonly("smoothing_status", &HybridAStar::Stats::smoothingStatus);

	py::class_<HybridAStar, PathPlannerSE2Base>(m, "HybridAStar")
		.def(py::init<>())
		.def(py::init<const HybridAStar::SearchParameters&>())
		.def(py::init<const HybridAStar::SearchParameters&, int, int>(), py::arg("parameters"), py::arg("max_batch"), py::arg("max_nodes") = 81920)
		.def("initialize", &HybridAStar::Initialize)
		.def_readwrite("path_interpolation", &HybridAStar::pathInterpolation)
		.def("get_stats", &HybridAStar::GetStats)
		.def("get_graph_search_optimal_cost", &HybridAStar::GetGraphSearchOptimalCost)
		.def("get_graph_search_path", &HybridAStar::GetGraphSearchPath)
		.def("get_graph_search_nodes", &HybridAStar::GetGraphSearchNodes)
		.def("get_graph_search_explored_path_set", &HybridAStar::GetGraphSearchExploredPathSet)
		.def("visualize_obstacle_heuristic", &HybridAStar::VisualizeObstacleHeuristic)
		.def("get_smoothed_path", &HybridAStar::GetSmoothedPath)
		.def_property("smoother_parameters", &HybridAStar::GetSmootherParameters, &HybridAStar::SetSmootherParameters)
		.def("get_search_parameters", &HybridAStar::GetSearchParameters)
		.def("set_seed", &HybridAStar::SetSeed)
		// heuristic clearance (include/pp_hip.h): the obstacle heuristic also blocks cells with !(dist >= radius); 0 = the reference's rule
		.def("set_heuristic_clearance", &HybridAStar::SetHeuristicClearance, py::arg("radius"))
		.def_property_readonly("heuristic_clearance", &HybridAStar::GetHeuristicClearance)
		.def("search_batch",
			[](HybridAStar& h, py::array_t<double, py::array::c_style | py::array::forcecast> starts, py::array_t<double, py::array::c_style | py::array::forcecast> goals,
				py::array_t<uint64_t, py::array::c_style | py::array::forcecast> seeds) {
				const size_t n = starts.shape(0);
				std::vector<Pose2d> s(n), g(n);
				std::vector<uint64_t> sd(seeds.data(), seeds.data() + n);
				for (size_t i = 0; i < n; i++) {
					s[i] = Pose2d(starts.at(i, 0), starts.at(i, 1), starts.at(i, 2));
					g[i] = Pose2d(goals.at(i, 0), goals.at(i, 1), goals.at(i, 2));
				}
				auto res = h.SearchBatch(s, g, sd);
				py::list out;
				for (size_t i = 0; i < n; i++)
					out.append(py::make_tuple(res[i].status, res[i].cost, res[i].n_expanded, res[i].n_path));
				return out;
			});

	// ---- the streaming pipeline (beyond the reference's surface): HybridAStar::SearchPath for a stream of queries, paths by ticket ----
	py::class_<HybridAStarPipeline>(m, "HybridAStarPipeline")
		.def(py::init<const HybridAStar::SearchParameters&, int, int, int>(), py::arg("parameters"), py::arg("capacity") = 24576, py::arg("max_nodes") = 81920,
			py::arg("search_rows") = 0)
		.def("initialize", &HybridAStarPipeline::Initialize)
		.def("submit",
			[](HybridAStarPipeline& h, const std::vector<Pose2d>& starts, const std::vector<Pose2d>& goals, const std::vector<uint64_t>& seeds) {
				std::vector<uint64_t> tickets;
				h.Submit(starts, goals, seeds, &tickets);
				return tickets; // of the prefix taken
			})
		// completed queries as (ticket, status, cost, n_expanded, n_path); hold=True keeps their slots for get_path / post_process until release
		.def("poll",
			[](HybridAStarPipeline& h, int maxResults, bool hold) {
				std::vector<HybridAStarPipeline::Result> res;
				h.Poll(res, maxResults, hold);
				py::list out;
				for (const auto& r : res)
					out.append(py::make_tuple(r.ticket, r.status, r.cost, r.numExpanded, r.numPathNodes));
				return out;
			},
			py::arg("max_results") = 4096, py::arg("hold") = false)
		.def("post_process", &HybridAStarPipeline::PostProcess, py::arg("tickets"), py::arg("path_interpolation") = 0.1f)
		// held plans against a map as it is now: (status, n_edges, blocked_edge, blocked_ratio, valid_length, length) per ticket; status 0 still valid,
		// 1 an edge is blocked, 2 only the goal pose fails, -1 no plan.  validator=None: the pipeline's own validator and map
		.def("revalidate",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const Ref<StateValidatorOccupancyMap>& validator) {
				py::list out;
				for (const auto& r : h.Revalidate(tickets, validator))
					out.append(py::make_tuple((int)r.verdict, r.numEdges, r.blockedEdge, r.blockedRatio, r.validLength, r.length));
				return out;
			},
			py::arg("tickets"), py::arg("validator") = Ref<StateValidatorOccupancyMap>())
		// held plans stamped into a map's occupancy grid: (status, n_samples, (row_min, row_max, col_min, col_max), length) per ticket.  validator=None: the
		// pipeline's own validator's map (refused with queries in flight)
		.def("stamp",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const Ref<StateValidatorOccupancyMap>& validator, double spacing, float margin,
				const std::vector<int32_t>& values, const std::vector<double>& fromLength, const std::vector<double>& toLength) {
				py::list out;
				for (const auto& r : h.Stamp(tickets, validator, spacing, margin, values, fromLength, toLength))
					out.append(py::make_tuple((int)r.status, r.numSamples, py::make_tuple(r.rowMin, r.rowMax, r.colMin, r.colMax), r.length));
				return out;
			},
			py::arg("tickets"), py::arg("validator") = Ref<StateValidatorOccupancyMap>(), py::arg("spacing") = 0.1, py::arg("margin") = 0.0f,
			py::arg("values") = std::vector<int32_t>(), py::arg("from_length") = std::vector<double>(), py::arg("to_length") = std::vector<double>())
		// vehicles located on their held plans: (status, edge, direction, n_samples, s, ratio, distance, along, lateral, heading_error, length, pose) per ticket
		.def("locate",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const std::vector<Pose2d>& poses, double spacing, double headingWeight,
				const std::vector<double>& fromLength, const std::vector<double>& toLength) {
				py::list out;
				for (const auto& r : h.Locate(tickets, poses, spacing, headingWeight, fromLength, toLength))
					out.append(py::make_tuple((int)r.status, r.edge, r.direction, r.numSamples, r.s, r.ratio, r.distance, r.along, r.lateral, r.headingError, r.length, r.pose));
				return out;
			},
			py::arg("tickets"), py::arg("poses"), py::arg("spacing") = 0.1, py::arg("heading_weight") = 0.0, py::arg("from_length") = std::vector<double>(),
			py::arg("to_length") = std::vector<double>())
		// speeds and arrival times along held plans: ((status, n_samples, n_cusps, length, s_first, s_last, duration, v_peak, min_clearance, s_min_clearance), s, v, t) per
		// ticket; validator=None: the pipeline's own validator's map, read only when clearance_gain > 0
		.def("speed_profile",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, double spacing, double vMaxForward, double vMaxReverse, double aAcc, double aDec, double aLat, double dwell,
				double clearanceGain, double vFloor, int maxSamples, const std::vector<double>& fromLength, const std::vector<double>& toLength, const std::vector<double>& vStart,
				const std::vector<double>& vEnd, const Ref<StateValidatorOccupancyMap>& validator) {
				HybridAStarPipeline::SpeedLimits limits;
				limits.vMaxForward = vMaxForward;
				limits.vMaxReverse = vMaxReverse;
				limits.aAcc = aAcc;
				limits.aDec = aDec;
				limits.aLat = aLat;
				limits.dwell = dwell;
				limits.clearanceGain = clearanceGain;
				limits.vFloor = vFloor;
				py::list out;
				for (const auto& r : h.SpeedProfile(tickets, spacing, limits, maxSamples, fromLength, toLength, vStart, vEnd, validator))
					out.append(py::make_tuple(py::make_tuple((int)r.status, r.numSamples, r.numCusps, r.length, r.sFirst, r.sLast, r.duration, r.vPeak, r.minClearance, r.sMinClearance), r.s,
						r.v, r.t));
				return out;
			},
			py::arg("tickets"), py::arg("spacing") = 0.1, py::arg("v_max_forward") = 5.0, py::arg("v_max_reverse") = 2.0, py::arg("a_acc") = 1.5, py::arg("a_dec") = 2.5,
			py::arg("a_lat") = 2.0, py::arg("dwell") = 0.0, py::arg("clearance_gain") = 0.0, py::arg("v_floor") = 0.0, py::arg("max_samples") = 2048,
			py::arg("from_length") = std::vector<double>(), py::arg("to_length") = std::vector<double>(), py::arg("v_start") = std::vector<double>(),
			py::arg("v_end") = std::vector<double>(), py::arg("validator") = Ref<StateValidatorOccupancyMap>())
		.def("conflicts",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const std::vector<double>& tStart, const py::object& pairs, double tFrom, double tTo, double dt,
				double margin, bool holdBefore, bool holdAfter, bool poses) {
				HybridAStarPipeline::ConflictHorizon horizon;
				horizon.tFrom = tFrom;
				horizon.tTo = tTo;
				horizon.dt = dt;
				horizon.margin = margin;
				horizon.holdBefore = holdBefore;
				horizon.holdAfter = holdAfter;
				const bool all = pairs.is_none();
				const auto r = h.Conflicts(tickets, tStart, all ? std::vector<std::pair<int, int>>() : pairs.cast<std::vector<std::pair<int, int>>>(), all, horizon, poses);
				py::list plans, found, xyt;
				for (const auto& p : r.plans) {
					plans.append(py::make_tuple((int)p.status, p.numPresent, p.first, p.last, p.sEnter, p.sLeave));
					if (poses) {
						py::list one;
						for (const Pose2d& q : p.poses)
							one.append(py::make_tuple(q.x(), q.y(), q.theta));
						xyt.append(one);
					}
				}
				for (const auto& c : r.pairs)
					found.append(py::make_tuple((int)c.status, c.numTimes, c.numConflict, c.tFirst, py::make_tuple(c.sFirst[0], c.sFirst[1]), c.minSeparation, c.tMin,
						py::make_tuple(c.sMin[0], c.sMin[1])));
				return poses ? py::object(py::make_tuple(plans, found, xyt)) : py::object(py::make_tuple(plans, found));
			},
			"Space-time conflicts between held queries on the timetables of the last speed_profile call.  tickets: the held queries; t_start: the absolute time each starts "
			"to drive, one per ticket; pairs: (i, j) indices into tickets, None: every i < j in row-major order; t_from, t_to: the horizon in absolute seconds; dt: the step of "
			"the global time lattice k * dt; margin: conflict iff the separation of the vehicles' discs is below it; hold_before / hold_after: a vehicle stands at its first / "
			"last sample before its start / behind its end instead of being absent; poses: also return every plan's (x, y, theta) per lattice time (NaN where absent).  Returns "
			"(plans, pairs[, poses]): per plan (status, n_present, first, last, s_enter, s_leave), per pair (status, n_times, n_conflict, t_first, s_first, min_separation, "
			"t_min, s_min).",
			py::arg("tickets"), py::arg("t_start"), py::arg("pairs") = py::none(), py::arg("t_from") = 0.0, py::arg("t_to") = 60.0, py::arg("dt") = 0.1, py::arg("margin") = 0.0,
			py::arg("hold_before") = false, py::arg("hold_after") = false, py::arg("poses") = false)
		.def("deconflict",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const std::vector<double>& tStart, const py::object& pairs, double tFrom, double tTo, double dt,
				double margin, bool holdBefore, bool holdAfter, int maxDelaySteps) {
				HybridAStarPipeline::ConflictHorizon horizon;
				horizon.tFrom = tFrom;
				horizon.tTo = tTo;
				horizon.dt = dt;
				horizon.margin = margin;
				horizon.holdBefore = holdBefore;
				horizon.holdAfter = holdAfter;
				const bool all = pairs.is_none();
				py::list out;
				for (const auto& d : h.Deconflict(tickets, tStart, all ? std::vector<std::pair<int, int>>() : pairs.cast<std::vector<std::pair<int, int>>>(), all, horizon, maxDelaySteps))
					out.append(py::make_tuple((int)d.status, d.delaySteps, d.numTried, d.blocker, d.tStart, d.tBlock, py::make_tuple(d.sBlock[0], d.sBlock[1])));
				return out;
			},
			"Start delays that clear conflicts between held queries, by priority, on the timetables of the last speed_profile call.  tickets: the held queries, highest "
			"priority first; t_start: the absolute time each would start to drive, one per ticket; pairs: (i, j) indices into tickets, of which the larger index yields, None: "
			"every pair; t_from, t_to: the horizon in absolute seconds; dt: the step of the global time lattice k * dt, and of the delays; margin: conflict iff the separation "
			"of the vehicles' discs is below it; hold_before / hold_after: a vehicle stands at its first / last sample before its start / behind its end instead of being "
			"absent; max_delay_steps: the largest delay tried, in lattice steps.  Returns per ticket (status, delay_steps, n_tried, blocker, t_start, t_block, s_block): "
			"status 0 scheduled with the effective start t_start, 1 no delay is clear (those below ignore it), -1 no speed profile.",
			py::arg("tickets"), py::arg("t_start"), py::arg("pairs") = py::none(), py::arg("t_from") = 0.0, py::arg("t_to") = 60.0, py::arg("dt") = 0.1, py::arg("margin") = 0.0,
			py::arg("hold_before") = false, py::arg("hold_after") = false, py::arg("max_delay_steps") = 0)
		.def("deconflict_waits",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const std::vector<double>& tStart, const py::object& pairs, const std::vector<bool>& noStartWait,
				const std::vector<std::pair<int, int>>& fixed, double tFrom, double tTo, double dt, double margin, bool holdBefore, bool holdAfter, int maxDelaySteps, int maxPlaces) {
				HybridAStarPipeline::ConflictHorizon horizon;
				horizon.tFrom = tFrom;
				horizon.tTo = tTo;
				horizon.dt = dt;
				horizon.margin = margin;
				horizon.holdBefore = holdBefore;
				horizon.holdAfter = holdAfter;
				const bool all = pairs.is_none();
				std::vector<HybridAStarPipeline::FixedWait> committed;
				for (const auto& f : fixed)
					committed.push_back(HybridAStarPipeline::FixedWait { f.first, f.second });
				py::list out;
				for (const auto& w : h.DeconflictWaits(tickets, tStart, all ? std::vector<std::pair<int, int>>() : pairs.cast<std::vector<std::pair<int, int>>>(), all, horizon,
						 maxDelaySteps, maxPlaces, noStartWait, committed))
					out.append(py::make_tuple((int)w.status, w.place, w.row, w.waitSteps, w.numTried, w.blocker, w.tStart, w.tHold, w.tResume, w.sWait, w.tBlock,
						py::make_tuple(w.sBlock[0], w.sBlock[1])));
				return out;
			},
			"Waits at the start or at a timetable's stops that clear conflicts between held queries, by priority, on the timetables of the last speed_profile call: "
			"deconflict with the first max_places stops every plan reaches inside the horizon as further candidates.  tickets, t_start, pairs, t_from, t_to, dt, margin, "
			"hold_before, hold_after and max_delay_steps are deconflict's; no_start_wait: per ticket whether it may NOT wait at its start (empty: everybody may); fixed: per "
			"ticket a committed wait (row, steps) with row -2 free, -1 the start, >= 0 a stop's row (empty: everybody is free); max_places: stops listed per vehicle.  Returns "
			"per ticket (status, place, row, wait_steps, n_tried, blocker, t_start, t_hold, t_resume, s_wait, t_block, s_block): status 0 scheduled, 1 no candidate is clear, "
			"2 a fixed wait in conflict, -1 no speed profile, -2 the fixed row is no stop reached in time.",
			py::arg("tickets"), py::arg("t_start"), py::arg("pairs") = py::none(), py::arg("no_start_wait") = std::vector<bool>(),
			py::arg("fixed") = std::vector<std::pair<int, int>>(), py::arg("t_from") = 0.0, py::arg("t_to") = 60.0, py::arg("dt") = 0.1, py::arg("margin") = 0.0,
			py::arg("hold_before") = false, py::arg("hold_after") = false, py::arg("max_delay_steps") = 0, py::arg("max_places") = 0)
		.def("deconflict_tracks",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const std::vector<double>& tStart,
				const std::vector<std::pair<double, std::vector<std::tuple<double, double, double>>>>& tracks, const py::object& pairs, double tFrom, double tTo, double dt, double margin,
				bool holdBefore, bool holdAfter, int maxDelaySteps, bool details) {
				HybridAStarPipeline::ConflictHorizon horizon;
				horizon.tFrom = tFrom;
				horizon.tTo = tTo;
				horizon.dt = dt;
				horizon.margin = margin;
				horizon.holdBefore = holdBefore;
				horizon.holdAfter = holdAfter;
				std::vector<HybridAStarPipeline::Track> movers;
				for (const auto& k : tracks) {
					HybridAStarPipeline::Track t;
					t.radius = k.first;
					for (const auto& w : k.second)
						t.waypoints.push_back({ std::get<0>(w), std::get<1>(w), std::get<2>(w) });
					movers.push_back(std::move(t));
				}
				const bool all = pairs.is_none();
				const auto r = h.DeconflictTracks(tickets, tStart, movers, all ? std::vector<std::pair<int, int>>() : pairs.cast<std::vector<std::pair<int, int>>>(), all, horizon,
					maxDelaySteps, details);
				py::list out, found;
				for (const auto& d : r.plans)
					out.append(py::make_tuple((int)d.status, d.delaySteps, d.numTried, d.blocker, d.tStart, d.tBlock, py::make_tuple(d.sBlock[0], d.sBlock[1])));
				for (const auto& row : r.tracks) {
					py::list one;
					for (const auto& c : row)
						one.append(py::make_tuple((int)c.status, c.numTimes, c.numConflict, c.tFirst, c.sFirst, c.minSeparation, c.tMin, c.sMin));
					found.append(one);
				}
				return details ? py::object(py::make_tuple(out, found)) : py::object(out);
			},
			"deconflict with tracked movers: every vehicle takes the smallest start delay at which it is clear of the scheduled vehicles above it and of every track.  "
			"tracks: a list of (radius, [(t, x, y), ...]), discs that move along timed waypoints on straight lines, absent before the first and behind the last time, never "
			"delayed; the other arguments are deconflict's (pairs=[] and max_delay_steps=0: the plain check of each plan against the movers).  Returns per ticket deconflict's "
			"tuple -- a blocker >= len(tickets) names track blocker - len(tickets) -- and, with details, per ticket and track (status, n_times, n_conflict, t_first, s_first, "
			"min_separation, t_min, s_min) at the vehicle's reported candidate.",
			py::arg("tickets"), py::arg("t_start"), py::arg("tracks"), py::arg("pairs") = py::none(), py::arg("t_from") = 0.0, py::arg("t_to") = 60.0, py::arg("dt") = 0.1,
			py::arg("margin") = 0.0, py::arg("hold_before") = false, py::arg("hold_after") = false, py::arg("max_delay_steps") = 0, py::arg("details") = true)
		.def("candidate_pairs",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const std::vector<double>& tStart, int timesPerBox, int maxDelaySteps, bool boxes, const py::object& maxPairs,
				double tFrom, double tTo, double dt, double margin, bool holdBefore, bool holdAfter) {
				HybridAStarPipeline::ConflictHorizon horizon;
				horizon.tFrom = tFrom;
				horizon.tTo = tTo;
				horizon.dt = dt;
				horizon.margin = margin;
				horizon.holdBefore = holdBefore;
				horizon.holdAfter = holdAfter;
				const auto r = h.CandidatePairs(tickets, tStart, horizon, timesPerBox, maxDelaySteps, maxPairs.is_none() ? -1 : maxPairs.cast<int>(), boxes);
				py::list pairs, first, found;
				for (const auto& p : r.pairs)
					pairs.append(py::make_tuple(p.first, p.second));
				for (int b : r.firstBox)
					first.append(b);
				for (const auto& row : r.boxes) {
					py::list one;
					for (const auto& b : row)
						one.append(py::make_tuple(b.xMin, b.yMin, b.xMax, b.yMax));
					found.append(one);
				}
				py::dict summary;
				summary["n_found"] = r.numFound;
				summary["n_written"] = r.pairs.size();
				summary["n_boxes"] = r.numBoxes;
				summary["n_boxed"] = r.numBoxed;
				summary["reach"] = r.reach;
				return boxes ? py::tuple(py::make_tuple(pairs, first, summary, found)) : py::tuple(py::make_tuple(pairs, first, summary));
			},
			"the pairs of held plans that can meet at all, by a space-time broad phase: per ticket and block of times_per_box lattice times the bounding box of the vehicle's "
			"reference point under every start delay of 0 .. max_delay_steps steps (0 for a list meant for conflicts); a pair is listed when in some block its boxes are no "
			"further apart on either axis than margin and footprint allow.  Returns (pairs [(i, j), ...] ascending, first_box, summary dict with n_found, n_written, n_boxes, "
			"n_boxed and reach) and, with boxes, per ticket and box (xmin, ymin, xmax, ymax).  pairs feeds conflicts, deconflict and deconflict_tracks as it is; max_pairs=None: "
			"every pair the rule lists.  t_from, t_to, dt, margin, hold_before and hold_after are those of the call the list is meant for.",
			py::arg("tickets"), py::arg("t_start"), py::arg("times_per_box") = 64, py::arg("max_delay_steps") = 0, py::arg("boxes") = false, py::arg("max_pairs") = py::none(),
			py::arg("t_from") = 0.0, py::arg("t_to") = 60.0, py::arg("dt") = 0.1, py::arg("margin") = 0.0, py::arg("hold_before") = false, py::arg("hold_after") = false)
		.def("timetable",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const std::vector<std::vector<double>>& values, const std::string& by, int maxStops) {
				if (by != "length" && by != "time")
					throw std::invalid_argument("timetable: by is \"length\" or \"time\"");
				const auto r = h.Timetable(tickets, values, by == "time", maxStops);
				py::list plans, stops, results;
				for (const auto& p : r) {
					py::dict plan;
					plan["status"] = (int)p.status;
					plan["n_samples"] = p.numSamples;
					plan["n_stops"] = p.numStops;
					plan["n_listed"] = p.stops.size();
					plan["s_first"] = p.sFirst;
					plan["s_last"] = p.sLast;
					plan["duration"] = p.duration;
					plans.append(plan);
					py::list listed, looked;
					for (const auto& st : p.stops)
						listed.append(py::make_tuple(st.row, st.s, st.tArrive, st.tDepart));
					for (const auto& u : p.lookUps) {
						py::dict d;
						d["status"] = (int)u.status;
						d["row"] = u.row;
						d["edge"] = u.edge;
						d["direction"] = u.direction;
						d["s"] = u.s;
						d["t"] = u.t;
						d["v"] = u.v;
						d["a"] = u.a;
						d["ratio"] = u.ratio;
						d["kappa"] = u.kappa;
						d["pose"] = py::make_tuple(u.pose.x(), u.pose.y(), u.pose.theta);
						d["next_stop"] = u.nextStop;
						d["s_to_stop"] = u.sToStop;
						d["t_to_stop"] = u.tToStop;
						d["t_remaining"] = u.tRemaining;
						looked.append(d);
					}
					stops.append(listed);
					results.append(looked);
				}
				return py::make_tuple(plans, stops, results);
			},
			"questions to the timetables the last speed_profile call left on the device: values holds one list per ticket (all of one length; empty: stops only) of arc "
			"lengths (by=\"length\") or seconds since the plan's start (by=\"time\").  Returns (plans, stops, results): per ticket a dict (status, n_samples, n_stops, "
			"n_listed, s_first, s_last, duration), the list of its first max_stops stops as (row, s, t_arrive, t_depart), and per value a dict (status 0 inside the "
			"profile, 1 before, 2 behind it, -1 no profile; row, edge, direction, s, t, v, a, ratio, kappa, pose, next_stop, s_to_stop, t_to_stop, t_remaining).",
			py::arg("tickets"), py::arg("values"), py::arg("by") = "length", py::arg("max_stops") = 16)
		.def("retime",
			[](HybridAStarPipeline& h, const std::vector<uint64_t>& tickets, const std::vector<std::tuple<int, int, double>>& holds) {
				std::vector<HybridAStarPipeline::Hold> list;
				for (const auto& [plan, row, seconds] : holds) {
					HybridAStarPipeline::Hold x;
					x.plan = plan;
					x.row = row;
					x.seconds = seconds;
					list.push_back(x);
				}
				py::list out;
				for (const auto& r : h.Retime(tickets, list)) {
					py::dict d;
					d["status"] = (int)r.status;
					d["n_holds"] = r.numHolds;
					d["first_row"] = r.firstRow;
					d["bad_hold"] = r.badHold;
					d["held"] = r.held;
					d["duration_before"] = r.durationBefore;
					d["duration"] = r.duration;
					out.append(d);
				}
				return out;
			},
			"decided waits written into the timetables the last speed_profile call left on the device: holds is a list of (plan, row, seconds), strictly ascending in "
			"(plan, row), plan an index into tickets and row a stop of that plan's profile in 1 .. N - 1; seconds is added to every t_k with k >= row, in place, so that "
			"conflicts, timetable, candidate_pairs and the deconflict calls see the wait.  Returns per ticket a dict (status 0 applied, -1 no profile, -2 a hold's row is "
			"no stop, -3 a hold would make a dwell negative; n_holds, first_row, bad_hold, held, duration_before, duration).",
			py::arg("tickets"), py::arg("holds"))
		.def("get_path", &HybridAStarPipeline::GetPath, py::arg("ticket"))
		.def("get_graph_search_path", &HybridAStarPipeline::GetGraphSearchPath, py::arg("ticket"))
		.def("get_smoothing_status", &HybridAStarPipeline::GetSmoothingStatus, py::arg("ticket"))
		.def("release", &HybridAStarPipeline::Release, py::arg("tickets"))
		.def("in_flight", &HybridAStarPipeline::InFlight)
		.def("free_slots", &HybridAStarPipeline::FreeSlots)
		.def_property("smoother_parameters", &HybridAStarPipeline::GetSmootherParameters, &HybridAStarPipeline::SetSmootherParameters)
		.def("set_heuristic_clearance", &HybridAStarPipeline::SetHeuristicClearance, py::arg("radius"))
		.def_property_readonly("heuristic_clearance", &HybridAStarPipeline::GetHeuristicClearance);

	// ---- grid A* (pyplanning.cpp:124-197): cost / heuristic are Python callables per edge, as in the reference ----
	py::class_<NullAction>(m, "NullAction").def(py::init<>());
	using AStarHeuristicN2 = AStarHeuristic<GridCellPosition>;
	struct AStarHeuristicN2Wrapper : AStarHeuristicN2 {
		using AStarHeuristicN2::AStarHeuristicN2;
		double GetHeuristicValue(const GridCellPosition& state) override { PYBIND11_OVERRIDE_PURE(double, AStarHeuristicN2, GetHeuristicValue, state); }
		void SetGoal(const GridCellPosition& goal) override { PYBIND11_OVERRIDE_PURE(void, AStarHeuristicN2, SetGoal, goal); }
	};
	py::class_<AStarHeuristicN2, Ref<AStarHeuristicN2>, AStarHeuristicN2Wrapper>(m, "AStarHeuristicN2").def(py::init<>());
	py::class_<AStarHeuristicFcnN2, Ref<AStarHeuristicFcnN2>, AStarHeuristicN2>(m, "AStarHeuristicFcnN2").def(py::init<CellCostFcn>());
	py::class_<AverageHeuristic<GridCellPosition>, Ref<AverageHeuristic<GridCellPosition>>, AStarHeuristicN2>(m, "AverageHeuristicN2");

	using AStarStatePropagatorN2 = AStarStatePropagator<GridCellPosition>;
	struct AStarStatePropagatorN2Wrapper : AStarStatePropagatorN2 {
		using AStarStatePropagatorN2::AStarStatePropagatorN2;
		using ReturnType = std::vector<std::tuple<GridCellPosition, NullAction, double>>;
		ReturnType GetNeighborStates(const GridCellPosition& cell) override { PYBIND11_OVERRIDE_PURE(ReturnType, AStarStatePropagatorN2, GetNeighborStates, cell); }
	};
	py::class_<AStarStatePropagatorN2, Ref<AStarStatePropagatorN2>, AStarStatePropagatorN2Wrapper>(m, "AStarStatePropagatorN2").def(py::init<>());
	py::class_<AStarStatePropagatorFcnN2, Ref<AStarStatePropagatorFcnN2>, AStarStatePropagatorN2>(m, "AStarStatePropagatorFcnN2")
		.def(py::init<const Ref<OccupancyMap>&, const CellCostFcn&>());

	struct PathPlannerN2BaseWrapper : PathPlannerN2Base {
		using PathPlannerN2Base::PathPlannerN2Base;
		Status SearchPath() override { PYBIND11_OVERRIDE_PURE(Status, PathPlannerN2Base, SearchPath); }
		std::vector<GridCellPosition> GetPath() const override { PYBIND11_OVERRIDE_PURE(std::vector<GridCellPosition>, PathPlannerN2Base, GetPath); }
	};
	py::class_<PathPlannerN2Base, PathPlannerN2BaseWrapper>(m, "PathPlannerN2Base")
		.def(py::init<>())
		.def("search_path", &PathPlannerN2Base::SearchPath)
		.def("get_path", &PathPlannerN2Base::GetPath)
		.def("set_init_state", &PathPlannerN2Base::SetInitState)
		.def("set_goal_state", &PathPlannerN2Base::SetGoalState);
	py::class_<AStarN2, PathPlannerN2Base>(m, "AStarN2")
		.def(py::init<>())
		.def("initialize", &AStarN2::Initialize)
		.def("get_explored_states", &AStarN2::GetExploredStates)
		.def("get_expansion_order", &AStarN2::GetExpansionOrder)
		.def("get_optimal_cost", &AStarN2::GetOptimalCost);
	py::class_<BidirectionalAStarN2, PathPlannerN2Base>(m, "BidirectionalAStarN2")
		.def(py::init<>())
		.def_static("get_average_heuristic_pair", &BidirectionalAStarN2::GetAverageHeuristicPair)
		.def("initialize", &BidirectionalAStarN2::Initialize)
		.def("get_explored_states", &BidirectionalAStarN2::GetExploredStates)
		.def("get_expansion_orders", &BidirectionalAStarN2::GetExpansionOrders)
		.def("get_optimal_cost", &BidirectionalAStarN2::GetOptimalCost);

	// beyond the reference's module: the same two searches for many (init, goal) pairs on the device (Euclidean cost / heuristic)
	py::class_<GridSearchResult>(m, "GridSearchResult")
		.def_readonly("status", &GridSearchResult::status)
		.def_readonly("cost", &GridSearchResult::cost)
		.def_readonly("path", &GridSearchResult::path)
		.def_readonly("expanded", &GridSearchResult::expanded)
		.def_readonly("expanded_reverse", &GridSearchResult::expandedReverse);
	py::class_<GridAStarBatchHip>(m, "GridAStarBatch")
		.def(py::init<const Ref<OccupancyMap>&>())
		.def("search_batch",
			[](GridAStarBatchHip& self, const std::vector<GridCellPosition>& inits, const std::vector<GridCellPosition>& goals, bool bidirectional, bool wantExpanded) {
				return self.SearchBatch(inits, goals, bidirectional, wantExpanded);
			},
			py::arg("inits"), py::arg("goals"), py::arg("bidirectional") = false, py::arg("want_expanded") = false);

	py::class_<RRTParameters>(m, "RRTParameters")
		.def(py::init<>())
		.def_readwrite("max_iteration", &RRTParameters::maxIteration)
		.def_readwrite("max_number_tree_node", &RRTParameters::maxNumberTreeNode)
		.def_readwrite("max_connection_distance", &RRTParameters::maxConnectionDistance)
		.def_readwrite("goal_bias", &RRTParameters::goalBias);
	py::class_<RRTStarParameters>(m, "RRTStarParameters")
		.def(py::init<>())
		.def_readwrite("max_iteration", &RRTStarParameters::maxIteration)
		.def_readwrite("max_number_tree_node", &RRTStarParameters::maxNumberTreeNode)
		.def_readwrite("max_connection_distance", &RRTStarParameters::maxConnectionDistance)
		.def_readwrite("goal_bias", &RRTStarParameters::goalBias)
		.def_readwrite("rewire", &RRTStarParameters::rewire)
		.def_readwrite("radius_gamma", &RRTStarParameters::radiusGamma);
	py::class_<RRTR2>(m, "RRTR2")
		.def(py::init<const Point2d&, const Point2d&, const Ref<StateValidatorOccupancyMap>&>(), py::arg("lower"), py::arg("upper"), py::arg("validator") = nullptr)
		.def("set_parameters", &RRTR2::SetParameters)
		.def("set_seed", &RRTR2::SetSeed)
		.def("set_init_state", &RRTR2::SetInitState)
		.def("set_goal_state", &RRTR2::SetGoalState)
		.def("search_path", &RRTR2::SearchPath)
		.def("get_path", &RRTR2::GetPath);
	py::class_<RRTStarR2>(m, "RRTStarR2")
		.def(py::init<const Point2d&, const Point2d&, const Ref<StateValidatorOccupancyMap>&>(), py::arg("lower"), py::arg("upper"), py::arg("validator") = nullptr)
		.def("set_parameters", &RRTStarR2::SetParameters)
		.def("set_seed", &RRTStarR2::SetSeed)
		.def("set_init_state", &RRTStarR2::SetInitState)
		.def("set_goal_state", &RRTStarR2::SetGoalState)
		.def("search_path", &RRTStarR2::SearchPath)
		.def("get_path", &RRTStarR2::GetPath);
}
