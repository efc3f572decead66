"""Host-side mirror of the reference's filter interface, backed by the HIP library.

`Amcl` has the surface of `beluga::Amcl` (beluga/include/beluga/algorithm/amcl_core.hpp:81-233) /
`beluga_ros::Amcl` (beluga_ros/include/beluga_ros/amcl.hpp:102-282): same constructor ingredients
(map, motion model params, sensor model params, AmclParams), `particles()`, `initialize(pose, covariance)`,
`update_map(map)`, `update(control_action, measurement)` returning `None` where the reference returns
`std::nullopt`, and `force_update()`.  Parameter classes carry the reference's field names and defaults.
All per-particle work happens in libbeluga_mcl.so on the GPU; this module only marshals arguments.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np

from . import capi


@dataclass
class AmclParams:
    """beluga::AmclParams (amcl_core.hpp:34-55) + beluga_ros spatial resolutions (beluga_ros/amcl.hpp:90-97)."""
    update_min_d: float = 0.25
    update_min_a: float = 0.2
    resample_interval: int = 1
    selective_resampling: bool = False
    min_particles: int = 500
    max_particles: int = 2000
    alpha_slow: float = 0.001
    alpha_fast: float = 0.1
    kld_epsilon: float = 0.05
    kld_z: float = 3.0
    spatial_resolution_x: float = 0.5
    spatial_resolution_y: float = 0.5
    spatial_resolution_theta: float = 10.0 * math.pi / 180.0


@dataclass
class DifferentialDriveModelParam:
    """motion/differential_drive_model.hpp:40-68."""
    rotation_noise_from_rotation: float
    rotation_noise_from_translation: float
    translation_noise_from_translation: float
    translation_noise_from_rotation: float
    distance_threshold: float = 0.01


@dataclass
class OmnidirectionalDriveModelParam:
    """motion/omnidirectional_drive_model.hpp:36-73."""
    rotation_noise_from_rotation: float
    rotation_noise_from_translation: float
    translation_noise_from_translation: float
    translation_noise_from_rotation: float
    strafe_noise_from_translation: float
    distance_threshold: float = 0.01


@dataclass
class StationaryModelParam:
    """motion/stationary_model.hpp:40-62 takes no parameters."""


@dataclass
class LikelihoodFieldModelParam:
    """sensor/likelihood_field_model_base.hpp:42-64."""
    max_obstacle_distance: float = 100.0
    max_laser_distance: float = 2.0
    z_hit: float = 0.5
    z_random: float = 0.5
    sigma_hit: float = 0.2
    model_unknown_space: bool = False
    only_obstacle_boundaries: bool = False


@dataclass
class LikelihoodFieldProbModelParam(LikelihoodFieldModelParam):
    """sensor/likelihood_field_prob_model.hpp:34 (= LikelihoodFieldModelBaseParam)."""


@dataclass
class BeamModelParam:
    """sensor/beam_model.hpp:43-58."""
    z_hit: float = 0.5
    z_short: float = 0.5
    z_max: float = 0.05
    z_rand: float = 0.05
    sigma_hit: float = 0.2
    lambda_short: float = 0.1
    beam_max_range: float = 60.0


@dataclass
class OccupancyGrid:
    """An OccupancyGrid2 (sensor/data/occupancy_grid.hpp:39-75): row-major int8 cells, resolution, origin, value traits."""
    cells: np.ndarray  # (H, W) int8
    resolution: float
    origin: Sequence[float] = (1.0, 0.0, 0.0, 0.0)  # SE2 as (cos, sin, x, y)
    value_traits: Tuple[int, int, int] = (0, -1, 100)  # free, unknown, occupied


# kDefaultNeighborKernel2d (ndt_sensor_model.hpp:113-123), in its order
NDT_DEFAULT_KERNEL = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1))


@dataclass
class NDTModelParam2d:
    """beluga::NDTModelParam2d (sensor/ndt_sensor_model.hpp:153-166); ndt_amcl_node's defaults are 0.01 / 1.0 / 0.6."""
    minimum_likelihood: float = 0.0
    d1: float = 1.0
    d2: float = 1.0
    neighbors_kernel: Sequence[Tuple[int, int]] = NDT_DEFAULT_KERNEL


@dataclass
class NDTMap2d:
    """A SparseValueGrid2 of NDTCell2d (the layout of io::load_from_hdf5): integer keys cells[n,2], means[n,2], covariances[n,2,2]
    and the resolution; a cell's key is floor(p / resolution) of the points it covers (no origin)."""
    cells: np.ndarray
    means: np.ndarray
    covariances: np.ndarray
    resolution: float

    @classmethod
    def from_points(cls, points, resolution: float) -> "NDTMap2d":
        """The map of a point cloud (world frame) by the rule of detail::to_cells (ndt_sensor_model.hpp:88-110), on the host: keys by
        (p / resolution) truncated toward zero, cells of 5 points or more, in ascending (x, y) key order, fitted by the library's
        mcl_ndt_measurement_cells.  No device needed; Amcl.build_ndt_map builds the same cells on the device."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        means, covs = ndt_measurement_cells(pts, resolution)
        q = pts / float(resolution)
        q = q[np.all(np.abs(q) < 2147483647.0, axis=1)]  # (the others have no key: the fit drops them too)
        keys, counts = np.unique(q.astype(np.int32), axis=0, return_counts=True)  # rows in ascending (x, y) order
        keys = keys[counts >= 5].reshape(-1, 2)
        if len(keys) != len(means):
            raise RuntimeError("NDTMap2d.from_points: the keys and the fitted cells differ in number")
        return cls(cells=keys.astype(np.int32), means=means, covariances=covs, resolution=float(resolution))

    @classmethod
    def from_occupancy_grid(cls, grid: "OccupancyGrid", resolution: float) -> "NDTMap2d":
        """The same from the centres of the grid's occupied cells (occupied_cell_centres)."""
        return cls.from_points(occupied_cell_centres(grid), resolution)


def occupied_cell_centres(grid: "OccupancyGrid") -> np.ndarray:
    """The centres of a grid's occupied cells in the world frame, origin * (resolution * (index + 0.5)), in row-major order: the
    points mcl_build_ndt_map_from_grid fits, with its arithmetic."""
    yi, xi = np.nonzero(np.asarray(grid.cells) == grid.value_traits[2])
    c, s, ox, oy = (float(v) for v in grid.origin)
    lx, ly = (xi + 0.5) * float(grid.resolution), (yi + 0.5) * float(grid.resolution)
    return np.stack([(c * lx - s * ly) + ox, (s * lx + c * ly) + oy], 1)


@dataclass
class LandmarkModelParam:
    """beluga::LandmarkModelParam (sensor/landmark_sensor_model.hpp:44-48)."""
    sigma_range: float = 1.0
    sigma_bearing: float = 1.0
    random_prob: float = 1e-4


@dataclass
class BearingModelParam:
    """beluga::BearingModelParam (sensor/bearing_sensor_model.hpp:42-45); the pose in Sophus::SE3d::data() order: quaternion x, y, z, w,
    translation x, y, z."""
    sigma_bearing: float = 1.0
    sensor_pose_in_robot: Sequence[float] = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


@dataclass
class LandmarkPositionDetection:
    """types/landmark_detection_types.hpp:39-42; as a map entry the position is in the world frame."""
    detection_position_in_robot: Sequence[float]
    category: int


@dataclass
class LandmarkBearingDetection:
    """types/landmark_detection_types.hpp:45-48."""
    detection_bearing_in_sensor: Sequence[float]
    category: int


@dataclass
class LandmarkMapBoundaries:
    """Eigen::AlignedBox3d (types/landmark_detection_types.hpp:36)."""
    min: Sequence[float]
    max: Sequence[float]


class LandmarkMap:
    """beluga::LandmarkMap (sensor/data/landmark_map.hpp:40-75): LandmarkMap(boundaries, landmarks) or LandmarkMap(landmarks), whose
    boundaries are the landmarks' bounding box.  landmarks: LandmarkPositionDetection entries, or a (positions[n,3], categories[n]) pair."""

    def __init__(self, *args):
        if len(args) == 2 and isinstance(args[0], LandmarkMapBoundaries):
            boundaries, landmarks = args
        elif len(args) == 1:
            boundaries, landmarks = None, args[0]
        else:
            raise TypeError("LandmarkMap(boundaries, landmarks) or LandmarkMap(landmarks)")
        self.positions, self.categories = _detection_arrays(landmarks, "detection_position_in_robot")
        if boundaries is None and len(self.positions):
            boundaries = LandmarkMapBoundaries(self.positions.min(axis=0), self.positions.max(axis=0))
        self.boundaries = boundaries  # (None: the empty box of the reference's empty map, which the library refuses)

    def map_limits(self) -> Optional[LandmarkMapBoundaries]:
        return self.boundaries


def _detection_arrays(detections, attribute):
    """(vectors[n,3] float64, categories[n] uint32) of a list of detections or of a (vectors, categories) pair."""
    if isinstance(detections, tuple) and len(detections) == 2 and not hasattr(detections[0], "category"):
        xyz, cat = detections
    else:
        detections = list(detections)
        xyz = [getattr(d, attribute) for d in detections]
        cat = [d.category for d in detections]
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    cat = np.ascontiguousarray(cat, dtype=np.uint32).reshape(-1)
    if len(xyz) != len(cat):
        raise ValueError("vectors and categories differ in length")
    return xyz, cat


def _f64_rows(what, value, columns):
    """`value` as a C-contiguous float64 array of shape (n, columns), for Amcl.likelihoods*: an array of another dtype or another
    shape is refused here, before any library call (a sequence of Python floats is float64; nothing empty is refused)."""
    a = np.asarray(value)
    if a.size == 0:
        return np.zeros((0, columns), dtype=np.float64)
    if a.dtype != np.float64:
        raise TypeError(f"{what}: expected float64, got {a.dtype}")
    if a.ndim != 2 or a.shape[1] != columns:
        raise ValueError(f"{what}: expected shape (n, {columns}), got {a.shape}")
    return np.ascontiguousarray(a)


def _likelihood_detections(detections, attribute):
    """_detection_arrays with the checks of Amcl.likelihoods*: vectors (k, 3) float64, one category each."""
    if isinstance(detections, tuple) and len(detections) == 2 and not hasattr(detections[0], "category"):
        xyz = _f64_rows("detections", detections[0], 3)
        cat = np.asarray(detections[1])
        if cat.size and not np.issubdtype(cat.dtype, np.integer):
            raise TypeError(f"categories: expected integers, got {cat.dtype}")
        if cat.ndim > 1 or cat.size != len(xyz):
            raise ValueError("vectors and categories differ in length")
        if cat.size and (cat.min() < 0 or cat.max() > 0xFFFFFFFF):
            raise ValueError("categories: out of the range of uint32")
        return xyz, np.ascontiguousarray(cat, dtype=np.uint32).reshape(-1)
    return _detection_arrays(detections, attribute)


def _landmark_params_struct(p):
    if isinstance(p, LandmarkModelParam):
        return capi.LandmarkParams(p.sigma_range, p.sigma_bearing, p.random_prob)
    pose = [float(v) for v in p.sensor_pose_in_robot]
    if len(pose) != 7:
        raise ValueError("sensor_pose_in_robot takes 7 values (quaternion x, y, z, w, translation x, y, z)")
    return capi.BearingParams(p.sigma_bearing, (C.c_double * 7)(*pose))


def default_landmark_params() -> dict:
    p = capi.LandmarkParams()
    capi.load().mcl_default_landmark_params(C.byref(p))
    return {"sigma_range": p.sigma_range, "sigma_bearing": p.sigma_bearing, "random_prob": p.random_prob}


def default_bearing_params() -> dict:
    p = capi.BearingParams()
    capi.load().mcl_default_bearing_params(C.byref(p))
    return {"sigma_bearing": p.sigma_bearing, "sensor_pose_in_robot": tuple(p.sensor_pose_in_robot)}


def load_ndt_map_npz(path: str) -> NDTMap2d:
    """An NDT map saved as .npz with the HDF5 file's four datasets (cells, means, covariances, resolution)."""
    z = np.load(path)
    return NDTMap2d(cells=np.asarray(z["cells"], dtype=np.int32).reshape(-1, 2), means=np.asarray(z["means"], dtype=np.float64).reshape(-1, 2),
                    covariances=np.asarray(z["covariances"], dtype=np.float64).reshape(-1, 2, 2), resolution=float(z["resolution"]))


def ndt_params_struct(p: NDTModelParam2d) -> capi.NdtParams:
    kernel = list(p.neighbors_kernel)
    if not 1 <= len(kernel) <= capi.MCL_NDT_MAX_OFFSETS:
        raise ValueError(f"the neighbours kernel takes 1 .. {capi.MCL_NDT_MAX_OFFSETS} offsets")
    out = capi.NdtParams()
    out.minimum_likelihood, out.d1, out.d2 = p.minimum_likelihood, p.d1, p.d2
    out.num_offsets = len(kernel)
    for k, (dx, dy) in enumerate(kernel):
        out.offsets[2 * k], out.offsets[2 * k + 1] = int(dx), int(dy)
    return out


def default_ndt_params() -> dict:
    """mcl_default_ndt_params as a dict (minimum_likelihood, d1, d2, neighbors_kernel)."""
    p = capi.NdtParams()
    capi.load().mcl_default_ndt_params(C.byref(p))
    return {"minimum_likelihood": p.minimum_likelihood, "d1": p.d1, "d2": p.d2,
            "neighbors_kernel": tuple((p.offsets[2 * k], p.offsets[2 * k + 1]) for k in range(p.num_offsets))}


def ndt_measurement_cells(points_xy, resolution: float):
    """detail::to_cells (ndt_sensor_model.hpp:88-110) through the library: (means[k,2], covariances[k,2,2]) of the scan's cells."""
    pts = np.ascontiguousarray(points_xy, dtype=np.float64).reshape(-1, 2)
    cap = len(pts) // 5 + 1
    means, covs = np.zeros((cap, 2)), np.zeros((cap, 2, 2))
    k = C.c_uint64(0)
    st = capi.load().mcl_ndt_measurement_cells(_dp(pts), len(pts), float(resolution), _dp(means), _dp(covs), C.byref(k))
    if st != capi.MCL_OK:
        raise capi.MclError(st, "mcl_ndt_measurement_cells")
    return means[:k.value].copy(), covs[:k.value].copy()


def se2_from_xytheta(x: float, y: float, theta: float) -> np.ndarray:
    return np.array([math.cos(theta), math.sin(theta), x, y], dtype=np.float64)


def _dp(a: np.ndarray):
    return a.ctypes.data_as(capi.c_double_p)


class SharedMap:
    """One map on the device for any number of filters (mcl_shared_map_*): built once, for the device and the sensor model given -
    which every filter that uses it must share (the likelihood-field models: the same model and equal parameters) - and never
    changed.  Amcl.use_map attaches a filter to it.  close() gives up this object's reference only: the map lives until the last
    filter that uses it has left it.  field_build = 1: the field by the device's exact distance transform."""

    def __init__(self, grid: OccupancyGrid, sensor, *, device: int = 0, field_build: int = 0):
        self._lib = capi.load()
        self._map = None
        cfg = capi.Config()
        self._lib.mcl_default_config(C.byref(cfg))
        cfg.device_id = device
        if isinstance(sensor, LikelihoodFieldModelParam):
            cfg.sensor_kind = (capi.MCL_SENSOR_LIKELIHOOD_FIELD_PROB if isinstance(sensor, LikelihoodFieldProbModelParam)
                               else capi.MCL_SENSOR_LIKELIHOOD_FIELD)
            for k in ("max_obstacle_distance", "max_laser_distance", "z_hit", "z_random", "sigma_hit"):
                setattr(cfg.lf, k, getattr(sensor, k))
            cfg.lf.model_unknown_space = int(sensor.model_unknown_space)
            cfg.lf.only_obstacle_boundaries = int(sensor.only_obstacle_boundaries)
        elif isinstance(sensor, BeamModelParam):
            cfg.sensor_kind = capi.MCL_SENSOR_BEAM
        else:
            raise ValueError("SharedMap: sensor must be LikelihoodFieldModelParam, LikelihoodFieldProbModelParam or BeamModelParam")
        cells = np.ascontiguousarray(grid.cells, dtype=np.int8)
        H, W = cells.shape
        origin = np.ascontiguousarray(grid.origin, dtype=np.float64)
        traits = (C.c_int8 * 3)(*grid.value_traits)
        handle = capi._shared_map()
        st = self._lib.mcl_shared_map_create(C.byref(cfg), cells.ctypes.data_as(capi.c_i8_p), W, H, float(grid.resolution), _dp(origin),
                                             traits, int(field_build), C.byref(handle))
        if st != capi.MCL_OK:
            raise capi.MclError(st, self._lib.mcl_shared_map_last_error(None).decode())
        self._map = handle
        self.shape = (H, W)
        self.resolution = float(grid.resolution)

    def info(self) -> dict:
        """width, height, resolution, sensor_kind, device_id, device_bytes, host_bytes, users (filters attached now)."""
        if not self._map:
            raise ValueError("SharedMap: closed")
        out = capi.SharedMapInfo()
        st = self._lib.mcl_shared_map_get_info(self._map, C.byref(out))
        if st != capi.MCL_OK:
            raise capi.MclError(st, "mcl_shared_map_get_info")
        return {name: getattr(out, name) for name, _ in capi.SharedMapInfo._fields_}

    def close(self):
        if getattr(self, "_map", None):
            self._lib.mcl_shared_map_release(self._map)
            self._map = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class SearchHit:
    """A candidate of Amcl.global_search: pose (cos, sin, x, y), its score, id = cell * headings + heading, cell = y * width + x."""
    pose: np.ndarray
    score: float
    id: int
    cell: int
    heading: int


@dataclass
class LocalHit:
    """A seed's result of Amcl.local_search: the best lattice pose (cos, sin, x, y), its score, the seed's own score, the best's integer
    offsets, the number of candidates that share its score, and the score-weighted mean pose and covariance (x, y, theta) of the lattice
    with the ten sums they were formed from; moments_valid is False where the scores sum to 0 or to something not finite."""
    pose: np.ndarray
    score: float
    seed_score: float
    di: int
    dj: int
    dk: int
    plateau: int
    mean_pose: np.ndarray
    cov: np.ndarray
    sums: np.ndarray
    moments_valid: bool


class Amcl:
    def __init__(self, grid: OccupancyGrid, motion, sensor, params: AmclParams = AmclParams(), *,
                 seed: int = 0, device: int = 0, shard_offset: int = 0, shard_capacity: int = 0, hip_stream: int = 0,
                 options: Optional[dict] = None, ndt_small_cycle: bool = False, landmark_small_cycle: bool = False,
                 ndt_map_layout: int = 0):
        """options: library switches applied before the map is installed (mcl_set_option), e.g. {"field_build": 1} to build
        the likelihood field with the device's exact distance transform instead of the reference's wavefront on the host.
        ndt_small_cycle (NDT sensor model only): set_ndt_small_cycle(True) once the context exists.
        landmark_small_cycle (landmark and bearing sensor models only): set_landmark_small_cycle(True) likewise.
        ndt_map_layout (NDT sensor model only): set_ndt_map_layout(mode) before the first map is installed - 0 the dense index grid,
        1 the hashed table where the grid does not fit, 2 the hashed table always."""
        cfg = self._configure(grid, motion, sensor, params, seed=seed, device=device, shard_offset=shard_offset,
                              shard_capacity=shard_capacity, hip_stream=hip_stream, ndt_small_cycle=ndt_small_cycle,
                              landmark_small_cycle=landmark_small_cycle, ndt_map_layout=ndt_map_layout)
        ctx = capi._ctx()
        st = self._lib.mcl_create(C.byref(cfg), C.byref(ctx))
        if st != capi.MCL_OK:
            msg = self._lib.mcl_last_error(None).decode()
            self._ctx = None
            raise capi.MclError(st, msg)
        self._attach(ctx, grid, options, owned=True)

    def _configure(self, grid, motion, sensor, params, *, seed=0, device=0, shard_offset=0, shard_capacity=0, hip_stream=0,
                   ndt_small_cycle=False, landmark_small_cycle=False, ndt_map_layout=0):
        """The mcl_config of these constructor arguments (and what the object remembers of them)."""
        self._lib = capi.load()
        if ndt_small_cycle and not isinstance(sensor, NDTModelParam2d):
            raise ValueError("ndt_small_cycle needs the NDT sensor model (NDTModelParam2d)")
        self._ndt_small_cycle = bool(ndt_small_cycle)
        if ndt_map_layout and not isinstance(sensor, NDTModelParam2d):
            raise ValueError("ndt_map_layout needs the NDT sensor model (NDTModelParam2d)")
        self._ndt_map_layout = int(ndt_map_layout)
        if landmark_small_cycle and not isinstance(sensor, (LandmarkModelParam, BearingModelParam)):
            raise ValueError("landmark_small_cycle needs the landmark or the bearing sensor model")
        self._landmark_small_cycle = bool(landmark_small_cycle)
        cfg = capi.Config()
        self._lib.mcl_default_config(C.byref(cfg))
        cfg.device_id = device
        cfg.seed = seed
        for k in ("update_min_d", "update_min_a", "resample_interval", "min_particles", "max_particles", "alpha_slow",
                  "alpha_fast", "kld_epsilon", "kld_z", "spatial_resolution_x", "spatial_resolution_y", "spatial_resolution_theta"):
            setattr(cfg.amcl, k, getattr(params, k))
        cfg.amcl.selective_resampling = int(params.selective_resampling)
        if isinstance(motion, StationaryModelParam):
            cfg.motion_kind = capi.MCL_MOTION_STATIONARY
        else:
            for k in ("rotation_noise_from_rotation", "rotation_noise_from_translation", "translation_noise_from_translation",
                      "translation_noise_from_rotation", "distance_threshold"):
                setattr(cfg.motion, k, getattr(motion, k))
            if isinstance(motion, OmnidirectionalDriveModelParam):
                cfg.motion_kind = capi.MCL_MOTION_OMNIDIRECTIONAL
                cfg.strafe_noise_from_translation = motion.strafe_noise_from_translation
        if isinstance(sensor, LikelihoodFieldModelParam):
            cfg.sensor_kind = (capi.MCL_SENSOR_LIKELIHOOD_FIELD_PROB if isinstance(sensor, LikelihoodFieldProbModelParam)
                               else capi.MCL_SENSOR_LIKELIHOOD_FIELD)
            for k in ("max_obstacle_distance", "max_laser_distance", "z_hit", "z_random", "sigma_hit"):
                setattr(cfg.lf, k, getattr(sensor, k))
            cfg.lf.model_unknown_space = int(sensor.model_unknown_space)
            cfg.lf.only_obstacle_boundaries = int(sensor.only_obstacle_boundaries)
        elif isinstance(sensor, BeamModelParam):
            cfg.sensor_kind = capi.MCL_SENSOR_BEAM
            for k in ("z_hit", "z_short", "z_max", "z_rand", "sigma_hit", "lambda_short", "beam_max_range"):
                setattr(cfg.beam, k, getattr(sensor, k))
        elif isinstance(sensor, NDTModelParam2d):
            if not isinstance(grid, NDTMap2d):
                raise ValueError("the NDT sensor model takes an NDTMap2d")
            cfg.sensor_kind = capi.MCL_SENSOR_NDT
            self._ndt_params = sensor
        elif isinstance(sensor, (LandmarkModelParam, BearingModelParam)):
            if not isinstance(grid, LandmarkMap):
                raise ValueError("the landmark and bearing sensor models take a LandmarkMap")
            cfg.sensor_kind = capi.MCL_SENSOR_LANDMARK if isinstance(sensor, LandmarkModelParam) else capi.MCL_SENSOR_BEARING
            self._landmark_params = sensor
        else:
            raise ValueError("sensor must be LikelihoodFieldModelParam, BeamModelParam, NDTModelParam2d, LandmarkModelParam or BearingModelParam")
        if isinstance(grid, LandmarkMap) and not isinstance(sensor, (LandmarkModelParam, BearingModelParam)):
            raise ValueError("a LandmarkMap needs the landmark or the bearing sensor model")
        if isinstance(grid, NDTMap2d) and not isinstance(sensor, NDTModelParam2d):
            raise ValueError("an NDTMap2d needs the NDT sensor model (NDTModelParam2d)")
        cfg.shard_offset = shard_offset
        cfg.shard_capacity = shard_capacity
        cfg.hip_stream = hip_stream or None
        self.params = params
        self._cfg = cfg
        return cfg

    def _attach(self, ctx, grid, options, owned):
        """Binds the object to a created context.  owned = False: a member of an AmclBatch, which destroys it."""
        cfg = self._cfg
        self._ctx = ctx
        self._owned = owned
        self._shape = None
        self._est, self._info = capi.Estimate(), capi.UpdateInfo()
        self._est_ref, self._info_ref = C.byref(self._est), C.byref(self._info)
        self._est_view = np.frombuffer(self._est, dtype=np.float64, count=13)  # pose[4] | covariance[9]
        self._have_info = False
        self._landmark_kind = cfg.sensor_kind if cfg.sensor_kind in (capi.MCL_SENSOR_LANDMARK, capi.MCL_SENSOR_BEARING) else 0
        # a second handle of mcl_update that takes the arrays as raw addresses (no per-call pointer objects)
        self._update_fn = self._lib["mcl_update"]
        self._update_fn.restype = C.c_int32
        self._update_fn.argtypes = [capi._ctx, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        for name, value in (options or {}).items():
            self.set_option(name, value)
        if getattr(self, "_ndt_small_cycle", False):
            self.set_ndt_small_cycle(True)
        if getattr(self, "_landmark_small_cycle", False):
            self.set_landmark_small_cycle(True)
        if getattr(self, "_ndt_map_layout", 0):
            self.set_ndt_map_layout(self._ndt_map_layout)
        if grid is not None:  # (only a member of an AmclBatch may start without a map)
            self.update_map(grid)

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) and getattr(self, "_owned", True):
            self._lib.mcl_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != capi.MCL_OK:
            raise capi.MclError(st, self._lib.mcl_last_error(self._ctx).decode())

    # -- reference surface -------------------------------------------------------------------------
    def update_map(self, grid):
        """Amcl::update_map (amcl_core.hpp:150): an OccupancyGrid, an NDTMap2d for the NDT sensor model, or a LandmarkMap for the
        landmark and bearing sensor models."""
        if isinstance(grid, LandmarkMap):
            pos = np.ascontiguousarray(grid.positions, dtype=np.float64).reshape(-1, 3)
            cat = np.ascontiguousarray(grid.categories, dtype=np.uint32).reshape(-1)
            box = None
            if grid.boundaries is not None:
                box = np.concatenate([np.asarray(grid.boundaries.min, dtype=np.float64).reshape(3),
                                      np.asarray(grid.boundaries.max, dtype=np.float64).reshape(3)])
            sensor = getattr(self, "_landmark_params", None)
            prm = _landmark_params_struct(sensor) if sensor is not None else None
            self._check(self._lib.mcl_set_landmark_map(self._ctx, _dp(pos), cat.ctypes.data_as(capi.c_u32_p), len(pos),
                                                       _dp(box) if box is not None else None, C.byref(prm) if prm is not None else None))
            self._shape = None
            self._pending_shape = None
            return
        if isinstance(grid, NDTMap2d):
            keys = np.ascontiguousarray(grid.cells, dtype=np.int32).reshape(-1, 2)
            means = np.ascontiguousarray(grid.means, dtype=np.float64).reshape(-1, 2)
            covs = np.ascontiguousarray(grid.covariances, dtype=np.float64).reshape(-1, 4)
            if not (len(keys) == len(means) == len(covs)):
                raise ValueError("NDTMap2d: cells, means and covariances differ in length")
            prm = ndt_params_struct(getattr(self, "_ndt_params", None) or NDTModelParam2d())
            self._check(self._lib.mcl_set_ndt_map(self._ctx, keys.ctypes.data_as(C.POINTER(C.c_int32)), _dp(means), _dp(covs), len(keys),
                                                  float(grid.resolution), C.byref(prm)))
            self._ndt_resolution = float(grid.resolution)
            self._shape = None
            self._pending_shape = None
            return
        cells = np.ascontiguousarray(grid.cells, dtype=np.int8)
        H, W = cells.shape
        origin = np.ascontiguousarray(grid.origin, dtype=np.float64)
        traits = (C.c_int8 * 3)(*grid.value_traits)
        self._check(self._lib.mcl_set_map(self._ctx, cells.ctypes.data_as(capi.c_i8_p), W, H, float(grid.resolution), _dp(origin),
                                          traits))
        self._shape = (H, W)
        self._resolution = float(grid.resolution)
        self._pending_shape = None  # (a map given now replaces one that was still on its way)

    def use_map(self, shared: SharedMap):
        """update_map with a map that other filters read as well (mcl_use_shared_map): nothing is built or uploaded, and the filter's
        results are those of update_map with the same grid, bit for bit.  Raises MclError, and leaves the filter as it was, if the map
        was built for another device or sensor model."""
        if not shared._map:
            raise ValueError("SharedMap: closed")
        self._check(self._lib.mcl_use_shared_map(self._ctx, shared._map))
        self._shape = shared.shape
        self._resolution = shared.resolution
        self._pending_shape = None  # (a map given now replaces one that was still on its way)

    def build_ndt_map(self, source, resolution: float):
        """Extension (mcl_build_ndt_map_from_points / _from_grid): the NDT map built on the device from a point cloud (points[n,2], world
        frame) or from the occupied cells of an OccupancyGrid with the default value traits, and installed in place of the filter's map.
        The cells are NDTMap2d.from_points' bit for bit; the sensor model's parameters stay.  Read the result with ndt_map()."""
        if isinstance(source, OccupancyGrid):
            if tuple(source.value_traits) != (0, -1, 100):
                raise ValueError("build_ndt_map: the grid form takes the default value traits (occupied = 100)")
            cells = np.ascontiguousarray(source.cells, dtype=np.int8)
            H, W = cells.shape
            origin = np.ascontiguousarray(source.origin, dtype=np.float64)
            self._check(self._lib.mcl_build_ndt_map_from_grid(self._ctx, cells.ctypes.data_as(capi.c_i8_p), W, H, float(source.resolution),
                                                              _dp(origin), float(resolution)))
        else:
            pts = np.ascontiguousarray(source, dtype=np.float64).reshape(-1, 2)
            self._check(self._lib.mcl_build_ndt_map_from_points(self._ctx, _dp(pts), len(pts), float(resolution)))
        self._ndt_resolution = float(resolution)

    def ndt_map(self) -> NDTMap2d:
        """The NDT map the filter holds, however it was set (mcl_get_ndt_map)."""
        n = C.c_uint64(0)
        self._check(self._lib.mcl_get_ndt_map(self._ctx, None, None, None, 0, C.byref(n)))
        keys, means, covs = np.zeros((n.value, 2), dtype=np.int32), np.zeros((n.value, 2)), np.zeros((n.value, 2, 2))
        self._check(self._lib.mcl_get_ndt_map(self._ctx, keys.ctypes.data_as(C.POINTER(C.c_int32)), _dp(means), _dp(covs), n.value, C.byref(n)))
        return NDTMap2d(cells=keys, means=means, covariances=covs, resolution=self._ndt_resolution)

    def update_map_async(self, grid: OccupancyGrid):
        """Extension (mcl_set_map_async): the new map's likelihood field is built on a worker thread while the filter keeps running on
        the map it has; the swap happens at the start of the first update() after the build is done, or in map_commit()."""
        cells = np.ascontiguousarray(grid.cells, dtype=np.int8)
        H, W = cells.shape
        origin = np.ascontiguousarray(grid.origin, dtype=np.float64)
        traits = (C.c_int8 * 3)(*grid.value_traits)
        self._check(self._lib.mcl_set_map_async(self._ctx, cells.ctypes.data_as(capi.c_i8_p), W, H, float(grid.resolution), _dp(origin),
                                                traits))
        self._pending_shape = (H, W)
        self._pending_resolution = float(grid.resolution)

    def map_pending(self) -> int:
        """0: no map on its way, 1: its field is being built, 2: built, waiting for the swap."""
        v = C.c_int32(0)
        self._check(self._lib.mcl_map_pending(self._ctx, C.byref(v)))
        if v.value == 0 and getattr(self, "_pending_shape", None) is not None:
            self._shape, self._pending_shape = self._pending_shape, None
            self._resolution = self._pending_resolution
        return v.value

    def map_commit(self, wait: bool = True):
        """Swaps to the map given to update_map_async now (wait: for its build first; otherwise only if it is done)."""
        self._check(self._lib.mcl_map_commit(self._ctx, 1 if wait else 0))
        self.map_pending()

    def likelihood_field(self) -> np.ndarray:
        self.map_pending()  # (a swap inside update() may have changed the map's shape)
        """LikelihoodFieldModelBase::likelihood_field() (likelihood_field_model_base.hpp:102)."""
        out = np.zeros(self._shape, dtype=np.float32)
        self._check(self._lib.mcl_get_likelihood_field(self._ctx, out.ctypes.data_as(capi.c_float_p)))
        return out

    def set_likelihood_field(self, field: np.ndarray):
        field = np.ascontiguousarray(field, dtype=np.float32)
        assert field.shape == self._shape
        self._check(self._lib.mcl_set_likelihood_field(self._ctx, field.ctypes.data_as(capi.c_float_p)))

    def initialize(self, pose_xytheta, covariance):
        """Amcl::initialize(pose, covariance) (amcl_core.hpp:145-147). Raises RuntimeError on a bad covariance."""
        m = np.ascontiguousarray(pose_xytheta, dtype=np.float64)
        cv = np.ascontiguousarray(covariance, dtype=np.float64).reshape(9)
        st = self._lib.mcl_initialize_normal(self._ctx, _dp(m), _dp(cv))
        if st == capi.MCL_ERR_BAD_COVARIANCE:
            raise RuntimeError("Invalid covariance matrix")  # multivariate_normal_distribution.hpp:114-124
        self._check(st)

    def initialize_from_map(self):
        """beluga_ros::Amcl::initialize_from_map() (beluga_ros/include/beluga_ros/amcl.hpp:209): max_particles states drawn
        uniformly over the free cells of the map (random/multivariate_uniform_distribution.hpp:126-161)."""
        self._check(self._lib.mcl_initialize_from_map(self._ctx))

    def has_likelihood_field(self) -> bool:
        """beluga_ros::Amcl::has_likelihood_field() (amcl.hpp:181-188)."""
        v = C.c_int32(0)
        self._check(self._lib.mcl_has_likelihood_field(self._ctx, C.byref(v)))
        return bool(v.value)

    def likelihood_field_origin(self) -> np.ndarray:
        """beluga_ros::Amcl::likelihood_field_origin() (amcl.hpp:161-178) as (cos, sin, x, y); RuntimeError for the beam model."""
        out = np.zeros(4)
        st = self._lib.mcl_get_likelihood_field_origin(self._ctx, _dp(out))
        if st == capi.MCL_ERR_UNSUPPORTED:
            raise RuntimeError("The current sensor model does not support likelihood field")
        self._check(st)
        return out

    def update_point_cloud(self, control_action, points_xyz, origin_se3=(0, 0, 0, 1, 0, 0, 0)):
        """beluga_ros::Amcl::update(base_pose_in_odom, SparsePointCloud3f) (beluga_ros/src/amcl.cpp:67-81)."""
        ctrl = np.ascontiguousarray(control_action, dtype=np.float64)
        pts = np.ascontiguousarray(points_xyz, dtype=np.float32).reshape(-1, 3)
        origin = np.ascontiguousarray(origin_se3, dtype=np.float64)
        self._check(self._lib.mcl_update_point_cloud(self._ctx, _dp(ctrl), pts.ctypes.data_as(capi.c_float_p), len(pts), _dp(origin),
                                                     self._est_ref, self._info_ref))
        self._have_info = True
        if not self._info.updated:
            return None
        out = self._est_view.copy()
        return out[:4], out[4:13].reshape(3, 3)

    def set_particles(self, states, weights):
        """Amcl::initialize(distribution) with caller-drawn states (amcl_core.hpp:131-137)."""
        s = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 4)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        assert len(s) == len(w)
        self._check(self._lib.mcl_set_particles(self._ctx, _dp(s), _dp(w), len(w)))

    def num_particles(self) -> int:
        n = C.c_uint64(0)
        self._check(self._lib.mcl_num_particles(self._ctx, C.byref(n)))
        return n.value

    def particles(self):
        """Amcl::particles() (amcl_core.hpp:127): (states[n,4] as (cos,sin,x,y), weights[n])."""
        n = self.num_particles()
        s, w = np.zeros((n, 4)), np.zeros(n)
        got = C.c_uint64(0)
        self._check(self._lib.mcl_get_particles(self._ctx, _dp(s), _dp(w), n, C.byref(got)))
        return s, w

    def sample_particle_cloud(self, size: int, draw_id: int = 0) -> np.ndarray:
        """beluga_ros::assign_particle_cloud(particles, size, message) (particle_cloud.hpp:131-149): `size` states drawn
        with probability proportional to the weights, (size, 4) as (cos, sin, x, y); the set is not modified."""
        out = np.zeros((size, 4))
        if size:
            self._check(self._lib.mcl_sample_particle_cloud(self._ctx, size, draw_id, _dp(out)))
        return out if self.num_particles() else out[:0]

    def force_update(self):
        """Amcl::force_update() (amcl_core.hpp:204)."""
        self._check(self._lib.mcl_force_update(self._ctx))

    def update(self, control_action, measurement) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        """Amcl::update (amcl_core.hpp:165-201). Returns (pose (cos,sin,x,y), covariance 3x3) or None."""
        # This wrapper sits inside the measured cycle: no per-call ctypes objects, no dict, raw addresses for the arrays.
        if self._landmark_kind:
            return self._update_detections(control_action, measurement)
        ctrl = control_action if (type(control_action) is np.ndarray and control_action.dtype == np.float64
                                  and control_action.flags.c_contiguous) else np.ascontiguousarray(control_action, dtype=np.float64)
        pts = measurement if (type(measurement) is np.ndarray and measurement.dtype == np.float64
                              and measurement.flags.c_contiguous) else np.ascontiguousarray(measurement, dtype=np.float64)
        status = self._update_fn(self._ctx, ctrl.ctypes.data, pts.ctypes.data, pts.size // 2, self._est_ref, self._info_ref)
        if status != 0:
            self._check(status)
        self._have_info = True
        if not self._info.updated:
            return None
        out = self._est_view.copy()
        return out[:4], out[4:13].reshape(3, 3)

    def _update_detections(self, control_action, detections):
        """update(control, std::vector<LandmarkPositionDetection>) / (control, std::vector<LandmarkBearingDetection>)."""
        ctrl = np.ascontiguousarray(control_action, dtype=np.float64)
        landmark = self._landmark_kind == capi.MCL_SENSOR_LANDMARK
        xyz, cat = _detection_arrays(detections, "detection_position_in_robot" if landmark else "detection_bearing_in_sensor")
        fn = self._lib.mcl_update_landmarks if landmark else self._lib.mcl_update_bearings
        self._check(fn(self._ctx, _dp(ctrl), _dp(xyz), cat.ctypes.data_as(capi.c_u32_p), len(xyz), self._est_ref, self._info_ref))
        self._have_info = True
        if not self._info.updated:
            return None
        out = self._est_view.copy()
        return out[:4], out[4:13].reshape(3, 3)

    @property
    def last_info(self):
        """mcl_update_info of the last update as a dict (None before the first one)."""
        if not self._have_info:
            return None
        info = self._info
        return {
            "updated": bool(info.updated), "resampled": bool(info.resampled), "num_particles": info.num_particles,
            "weight_sum": info.weight_sum, "ess": info.effective_sample_size,
            "random_state_probability": info.random_state_probability,
        }

    def update_laser_scan(self, control_action, scan):
        """beluga_ros::Amcl::update(base_pose_in_odom, laser_scan) (beluga_ros/src/amcl.cpp:54-63)."""
        ctrl = np.ascontiguousarray(control_action, dtype=np.float64)
        self._check(self._lib.mcl_update_laser_scan(self._ctx, _dp(ctrl), C.byref(scan), self._est_ref, self._info_ref))
        self._have_info = True
        if not self._info.updated:
            return None
        out = self._est_view.copy()
        return out[:4], out[4:13].reshape(3, 3)

    # -- stage-level entry points (parity tests, multi-GPU driver) ------------------------------------
    def propagate(self, pose, previous_pose, step: int):
        a = np.ascontiguousarray(pose, dtype=np.float64)
        b = np.ascontiguousarray(previous_pose, dtype=np.float64)
        self._check(self._lib.mcl_propagate(self._ctx, _dp(a), _dp(b), step))

    def reweight(self, measurement):
        pts = np.ascontiguousarray(measurement, dtype=np.float64).reshape(-1, 2)
        self._check(self._lib.mcl_reweight(self._ctx, _dp(pts), len(pts)))

    def reweight_ndt_cells(self, means, covariances):
        """NDT model: w *= 1 + sum of likelihood_at(state * cell) over caller-fitted measurement cells (base frame)."""
        m = np.ascontiguousarray(means, dtype=np.float64).reshape(-1, 2)
        c = np.ascontiguousarray(covariances, dtype=np.float64).reshape(-1, 4)
        if len(m) != len(c):
            raise ValueError("reweight_ndt_cells: means and covariances differ in length")
        self._check(self._lib.mcl_reweight_ndt_cells(self._ctx, _dp(m), _dp(c), len(m)))

    def set_ndt_small_cycle(self, on: bool = True):
        """mcl_set_ndt_small_cycle: small NDT sets (up to 4096 particles) take the wave-per-particle reweight and the one-launch tail
        with one host synchronisation; a cycle that would inject random states is handed back to the host behind the policies.  In an
        AmclBatch such a member rides the fleet's shared launches.  Off by default; raises on another sensor model."""
        self._check(self._lib.mcl_set_ndt_small_cycle(self._ctx, int(bool(on))))

    def ndt_small_cycle(self) -> bool:
        on = C.c_int32(0)
        self._check(self._lib.mcl_get_ndt_small_cycle(self._ctx, C.byref(on)))
        return bool(on.value)

    def ndt_small_cycle_counts(self) -> Tuple[int, int]:
        """(small cycles that ended inside the one-launch tail, small cycles the tail handed back): running totals."""
        done, back = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.mcl_get_ndt_small_cycle_counts(self._ctx, C.byref(done), C.byref(back)))
        return done.value, back.value

    def set_ndt_map_layout(self, mode: int):
        """mcl_set_ndt_map_layout: how the NEXT update_map / build_ndt_map lays the NDT map out on the device - 0 the dense index grid
        over the keys' bounding box (the default; a box beyond 2^26 cells is refused), 1 the hashed table where that grid does not
        fit, 2 the hashed table always.  The same weights, bit for bit, on every map both layouts hold.  The installed map stays as
        it is.  Raises on another sensor model or another value."""
        self._check(self._lib.mcl_set_ndt_map_layout(self._ctx, int(mode)))

    def ndt_map_layout(self) -> Tuple[int, int]:
        """(mode, in_use): the mode as set, and what the installed map uses - 0 dense, 1 hashed, -1 no map."""
        mode, in_use = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.mcl_get_ndt_map_layout(self._ctx, C.byref(mode), C.byref(in_use)))
        return mode.value, in_use.value

    def set_landmark_small_cycle(self, on: bool = True):
        """mcl_set_landmark_small_cycle: small landmark and bearing sets (up to 4096 particles) take the wave-per-particle reweight and
        the one-launch tail with one host synchronisation.  In an AmclBatch such a member rides the fleet's shared launches
        (update_detections).  Off by default; raises on another sensor model."""
        self._check(self._lib.mcl_set_landmark_small_cycle(self._ctx, int(bool(on))))

    def landmark_small_cycle(self) -> bool:
        on = C.c_int32(0)
        self._check(self._lib.mcl_get_landmark_small_cycle(self._ctx, C.byref(on)))
        return bool(on.value)

    def reweight_landmarks(self, detections):
        """Landmark model: w *= product over the detections (LandmarkPositionDetection entries or a (positions, categories) pair)."""
        xyz, cat = _detection_arrays(detections, "detection_position_in_robot")
        self._check(self._lib.mcl_reweight_landmarks(self._ctx, _dp(xyz), cat.ctypes.data_as(capi.c_u32_p), len(xyz)))

    def reweight_bearings(self, detections):
        """Bearing model: w *= product over the detections (LandmarkBearingDetection entries or a (bearings, categories) pair)."""
        xyz, cat = _detection_arrays(detections, "detection_bearing_in_sensor")
        self._check(self._lib.mcl_reweight_bearings(self._ctx, _dp(xyz), cat.ctypes.data_as(capi.c_u32_p), len(xyz)))

    # -- the sensor model as a function: sensor_model(measurement)(state) at caller-given poses -----------------------------
    def likelihoods(self, poses, measurement) -> np.ndarray:
        """states | views::likelihoods(sensor_model(measurement)) (views/likelihoods.hpp:44-59): the factor by which a reweight with
        `measurement` would multiply the weight of a particle at each of `poses` - float64 (n, 4) as (cos, sin, x, y), in any order,
        anywhere on or off the map.  The filter is untouched.  measurement: the scan's points, float64 (B, 2), on a likelihood-field,
        beam or NDT filter; the detections - entries or a (vectors, categories) pair - on a landmark or bearing filter.  Wrong shapes
        and dtypes raise before the library is called."""
        p = _f64_rows("poses", poses, 4)
        out = np.empty(len(p), dtype=np.float64)
        if self._landmark_kind:
            landmark = self._landmark_kind == capi.MCL_SENSOR_LANDMARK
            xyz, cat = _likelihood_detections(measurement, "detection_position_in_robot" if landmark else "detection_bearing_in_sensor")
            fn = self._lib.mcl_likelihoods_landmarks if landmark else self._lib.mcl_likelihoods_bearings
            self._check(fn(self._ctx, _dp(p), len(p), _dp(xyz), cat.ctypes.data_as(capi.c_u32_p), len(xyz), _dp(out)))
            return out
        pts = _f64_rows("points", measurement, 2)
        self._check(self._lib.mcl_likelihoods(self._ctx, _dp(p), len(p), _dp(pts), len(pts), _dp(out)))
        return out

    def likelihoods_ndt_cells(self, poses, means, covariances) -> np.ndarray:
        """likelihoods() of an NDT filter from caller-fitted measurement cells (means (K, 2), covariances (K, 4) or (K, 2, 2))."""
        p = _f64_rows("poses", poses, 4)
        m = _f64_rows("means", means, 2)
        c = np.asarray(covariances)
        c = _f64_rows("covariances", c.reshape(len(c), 4) if c.ndim == 3 and c.shape[1:] == (2, 2) else c, 4)
        if len(m) != len(c):
            raise ValueError("likelihoods_ndt_cells: means and covariances differ in length")
        out = np.empty(len(p), dtype=np.float64)
        self._check(self._lib.mcl_likelihoods_ndt_cells(self._ctx, _dp(p), len(p), _dp(m), _dp(c), len(m), _dp(out)))
        return out

    def likelihoods_device(self, poses, points, out=None, synchronize: bool = True):
        """likelihoods() over torch tensors already on the filter's device: poses float64 (n, 4) contiguous, the scores into `out`
        (float64 (n,); made here if None), which is returned.  The points stay host memory.  What this saves is the two copies, not
        the waits: the work is enqueued on the FILTER's stream, which torch does not know, so the host first waits for torch's
        current stream (the tensors' producers) and, with synchronize (the default), for the filter's stream before the return -
        the default is fully synchronous.  synchronize=False drops the second wait: call sync() before reading `out` or handing
        it to torch.  A caller who needs no host wait at all orders the streams itself and calls mcl_likelihoods_device."""
        import torch

        if not isinstance(poses, torch.Tensor) or not poses.is_cuda:
            raise TypeError("poses: expected a torch tensor on the filter's device")
        if poses.device.index != self._cfg.device_id:
            raise ValueError(f"poses: on device {poses.device.index}, the filter is on device {self._cfg.device_id}")
        if poses.dtype != torch.float64:
            raise TypeError(f"poses: expected float64, got {poses.dtype}")
        if poses.dim() != 2 or poses.shape[1] != 4 or not poses.is_contiguous():
            raise ValueError(f"poses: expected a contiguous tensor of shape (n, 4), got {tuple(poses.shape)}")
        n = poses.shape[0]
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=poses.device)
        elif (not isinstance(out, torch.Tensor) or out.device != poses.device or out.dtype != torch.float64 or tuple(out.shape) != (n,)
              or not out.is_contiguous()):
            raise ValueError("out: expected a contiguous float64 tensor of shape (n,) on the poses' device")
        pts = _f64_rows("points", points, 2)
        torch.cuda.current_stream(poses.device).synchronize()
        self._check(self._lib.mcl_likelihoods_device(self._ctx, poses.data_ptr(), n, _dp(pts), len(pts), out.data_ptr()))
        if synchronize:
            self.sync()
        return out

    # -- ray casting as a function: the range the map predicts along a bearing from a pose (mcl_cast_rays*) ---------------------------
    @staticmethod
    def _cast_bearings(bearings, angles, points):
        """The (B, 2) table of (c, s) from exactly one of: bearings as they are; angles by numpy's cos and sin; scan points as
        (px / z, py / z) with z = sqrt(px * px + py * py), the beam model's own expressions, one rounding each."""
        if sum(v is not None for v in (bearings, angles, points)) != 1:
            raise ValueError("cast_rays: give exactly one of bearings, angles, points")
        if bearings is not None:
            return _f64_rows("bearings", bearings, 2)
        if angles is not None:
            a = np.asarray(angles, dtype=np.float64).reshape(-1)
            return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))
        p = _f64_rows("points", points, 2)
        z = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])
        with np.errstate(invalid="ignore", divide="ignore"):  # (a point of range 0 gives a NaN, which the library refuses)
            return np.ascontiguousarray(np.stack([p[:, 0] / z, p[:, 1] / z], axis=1))

    def cast_rays(self, poses, bearings=None, angles=None, points=None, max_range=None, hit_cells: bool = False, cells_visited: bool = False):
        """Ray2d::cast from each of `poses` - float64 (n, 4) as (cos, sin, x, y) - along each bearing: the ranges the map predicts,
        float64 (n, B); with hit_cells also the linear index y * width + x of each hit cell (int64 (n, B), -1 without a hit); with
        cells_visited also the cells the walks looked at, an int.  Returned alone or as a tuple in that order.  Give exactly one of
        bearings ((B, 2) unit vectors (c, s), used as they are), angles ((B,) radians in the pose's frame) and points ((B, 2) scan
        points: their bearings as the beam model forms them).  max_range: metres; default: the beam model's beam_max_range on a beam
        filter.  The filter is untouched.  Likelihood-field and beam filters."""
        p = _f64_rows("poses", poses, 4)
        table = self._cast_bearings(bearings, angles, points)
        if max_range is None:
            if self._cfg.sensor_kind != capi.MCL_SENSOR_BEAM:
                raise ValueError("cast_rays: max_range is needed (only a beam filter has one of its own)")
            max_range = self._cfg.beam.beam_max_range
        n, B = len(p), len(table)
        ranges = np.empty((n, B), dtype=np.float64)
        hits = np.empty((n, B), dtype=np.int64) if hit_cells else None
        visited = C.c_uint64(0)
        self._check(self._lib.mcl_cast_rays(self._ctx, _dp(p), n, _dp(table), B, float(max_range), _dp(ranges),
                                            hits.ctypes.data_as(capi.c_i64_p) if hit_cells else None, C.byref(visited) if cells_visited else None))
        result = (ranges,) + ((hits,) if hit_cells else ()) + ((int(visited.value),) if cells_visited else ())
        return result[0] if len(result) == 1 else result

    def expected_scan(self, pose_xytheta, angles, max_range=None) -> np.ndarray:
        """The scan the map predicts at (x, y, theta): the range along each of `angles` (radians in the robot's frame), float64 (B,)."""
        x, y, theta = (float(v) for v in pose_xytheta)
        pose = np.array([[math.cos(theta), math.sin(theta), x, y]], dtype=np.float64)
        return self.cast_rays(pose, angles=angles, max_range=max_range)[0]

    def cast_rays_device(self, poses, bearings=None, angles=None, points=None, max_range=None, hit_cells: bool = False,
                         cells_visited: bool = False, synchronize: bool = True):
        """cast_rays() over a torch tensor of poses already on the filter's device (float64 (n, 4), contiguous): the ranges, and with
        hit_cells the hit cells, come back as torch tensors on that device.  The bearings stay host memory.  The waits are
        likelihoods_device's: the host waits for torch's current stream first and, with synchronize (the default) or cells_visited,
        for the filter's stream before the return; with synchronize=False call sync() before reading the outputs."""
        import torch

        if not isinstance(poses, torch.Tensor) or not poses.is_cuda:
            raise TypeError("poses: expected a torch tensor on the filter's device")
        if poses.device.index != self._cfg.device_id:
            raise ValueError(f"poses: on device {poses.device.index}, the filter is on device {self._cfg.device_id}")
        if poses.dtype != torch.float64:
            raise TypeError(f"poses: expected float64, got {poses.dtype}")
        if poses.dim() != 2 or poses.shape[1] != 4 or not poses.is_contiguous():
            raise ValueError(f"poses: expected a contiguous tensor of shape (n, 4), got {tuple(poses.shape)}")
        table = self._cast_bearings(bearings, angles, points)
        if max_range is None:
            if self._cfg.sensor_kind != capi.MCL_SENSOR_BEAM:
                raise ValueError("cast_rays_device: max_range is needed (only a beam filter has one of its own)")
            max_range = self._cfg.beam.beam_max_range
        n, B = poses.shape[0], len(table)
        ranges = torch.empty((n, B), dtype=torch.float64, device=poses.device)
        hits = torch.empty((n, B), dtype=torch.int64, device=poses.device) if hit_cells else None
        visited = C.c_uint64(0)
        torch.cuda.current_stream(poses.device).synchronize()
        self._check(self._lib.mcl_cast_rays_device(self._ctx, poses.data_ptr(), n, _dp(table), B, float(max_range), ranges.data_ptr(),
                                                   hits.data_ptr() if hit_cells else None, C.byref(visited) if cells_visited else None))
        if synchronize:
            self.sync()
        result = (ranges,) + ((hits,) if hit_cells else ()) + ((int(visited.value),) if cells_visited else ())
        return result[0] if len(result) == 1 else result

    # -- range table for the beam model: the expected range as one look-up per beam in place of a walk (mcl_build_range_table) -------------
    def build_range_table(self, num_angles: int = 360):
        """Build the table of the current map - per cell and heading bin of `num_angles`, the squared cell distance to the cell the exact
        cast from the cell's centre hits - and switch update(), reweight() and likelihoods() over to it from the next reweight on.  An
        approximation (the source's position inside its cell and the heading within a bin are discarded), hence opt-in.  Whatever installs
        a map afterwards rebuilds the table.  width * height * num_angles * 4 bytes; refused above option range_table_max_bytes.  Beam
        filters only.  cast_rays() and global_search() stay exact."""
        self._check(self._lib.mcl_build_range_table(self._ctx, int(num_angles)))

    def drop_range_table(self):
        """Back to the exact walk; the table's memory is freed."""
        self._check(self._lib.mcl_drop_range_table(self._ctx))

    def range_table_info(self) -> dict:
        """built, num_angles, width, height, bytes, builds (tables built, rebuilds included), lut_launches (reweights that read a table)."""
        info = capi.RangeTableInfo()
        self._check(self._lib.mcl_range_table_get_info(self._ctx, C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in capi.RangeTableInfo._fields_}

    def range_table_bearings(self) -> np.ndarray:
        """The bins' bearings (cos, sin) the table was built with, float64 (A, 2)."""
        out = np.empty((self.range_table_info()["num_angles"], 2), dtype=np.float64)
        self._check(self._lib.mcl_range_table_bearings(self._ctx, _dp(out)))
        return out

    def range_table(self, first_cell: int = 0, num_cells: Optional[int] = None) -> np.ndarray:
        """The table as uint32: the whole of it as (H, W, A) - for small maps: it is copied to the host - or, with first_cell / num_cells,
        the rows of those cells (cell = y * W + x) as (num_cells, A).  0xFFFFFFFF: no hit."""
        info = self.range_table_info()
        whole = first_cell == 0 and num_cells is None
        count = info["width"] * info["height"] - first_cell if num_cells is None else int(num_cells)
        out = np.empty((max(count, 0), info["num_angles"]), dtype=np.uint32)
        self._check(self._lib.mcl_range_table_read(self._ctx, int(first_cell), count, out.ctypes.data_as(capi.c_u32_p)))
        return out.reshape(info["height"], info["width"], info["num_angles"]) if whole else out

    # -- global pose search: every free cell and heading scored by the sensor model, the best kept (mcl_global_search*) ------------
    def _search_params(self, cell_stride, headings, pool, max_results, separation_xy, separation_theta):
        """The facade's metres and radians as cells and heading steps, by round()."""
        headings = int(headings)
        if not (separation_xy >= 0.0 and math.isfinite(separation_xy) and separation_theta >= 0.0 and math.isfinite(separation_theta)):
            raise ValueError("global_search: a separation is negative or not finite")
        # One more call of the library per search, and harmless: a map given by update_map_async is swapped in inside an update(), and
        # map_pending() is where this object learns of it (_shape, _resolution).
        self.map_pending()
        resolution = getattr(self, "_resolution", None)
        if not resolution:
            raise ValueError("global_search: the filter has no occupancy grid whose resolution the separation could be counted in")
        cells = min(int(round(float(separation_xy) / resolution)), 0xFFFFFFFF)
        steps = min(int(round(float(separation_theta) / (2.0 * math.pi / headings))), 0xFFFFFFFF) if headings > 0 else 0
        return capi.SearchParams(int(cell_stride), headings, int(pool), int(max_results), cells, steps)

    @staticmethod
    def _search_hits(hits, count):
        return [SearchHit(np.array(h.pose, dtype=np.float64), h.score, h.id, h.cell, h.heading) for h in hits[:count]]

    def _search(self, fn, capacity, measurement, params):
        pts = _f64_rows("points", measurement, 2)
        hits = (capi.SearchHit * max(int(capacity), 1))()
        count = C.c_uint64(0)
        info = capi.SearchInfo()
        self._check(fn(self._ctx, _dp(pts), len(pts), C.byref(params), hits, int(capacity), C.byref(count), C.byref(info)))
        self.last_search_info = {name: getattr(info, name) for name, _ in capi.SearchInfo._fields_}
        return self._search_hits(hits, count.value)

    def global_search(self, measurement, cell_stride=2, headings=72, pool=1024, max_results=16, separation_xy=0.5,
                      separation_theta=math.radians(30)):
        """Localising without an initial guess: every free cell of the map whose x and y are multiples of cell_stride, at `headings`
        headings each, is scored with the sensor model on the device as likelihoods() would score it; of the best `pool` candidates those
        that lie neither within separation_xy (metres) nor within separation_theta (radians) of a better kept one are returned, best
        first, at most max_results SearchHit.  The filter is untouched.  Likelihood-field and beam filters; the scan's points (B, 2).
        last_search_info holds the call's counts."""
        params = self._search_params(cell_stride, headings, pool, max_results, separation_xy, separation_theta)
        return self._search(self._lib.mcl_global_search, params.max_results, measurement, params)

    def global_search_pool(self, measurement, cell_stride=2, headings=72, pool=1024):
        """The pool global_search chooses from, before the suppression: the best `pool` candidates by (score descending, id ascending)."""
        params = capi.SearchParams(int(cell_stride), int(headings), int(pool), 1, 0, 0)
        return self._search(self._lib.mcl_global_search_pool, params.pool, measurement, params)

    def search_candidates(self, cell_stride=2, headings=72, first=0, count=None):
        """The candidates as the device makes them, in id order: (ids uint64 (k,), poses float64 (k, 4), total).  count None: all."""
        params = capi.SearchParams(int(cell_stride), int(headings), 1, 1, 0, 0)
        total = C.c_uint64(0)
        if count is None:
            self._check(self._lib.mcl_global_search_candidates(self._ctx, C.byref(params), 0, 0, None, None, C.byref(total)))
            count = max(total.value - int(first), 0)
        ids = np.zeros(int(count), dtype=np.uint64)
        poses = np.zeros((int(count), 4), dtype=np.float64)
        self._check(self._lib.mcl_global_search_candidates(self._ctx, C.byref(params), int(first), int(count), ids.ctypes.data_as(capi.c_u64_p),
                                                           _dp(poses), C.byref(total)))
        k = min(int(count), max(total.value - int(first), 0))
        return ids[:k], poses[:k], total.value

    def relocalize(self, measurement, covariance=None, *, refine=None, **search):
        """global_search(measurement, **search), then initialize(best pose, covariance): host glue.  Returns the hits; with none
        (a map without a candidate cell) the filter is left as it was.
        refine: None, or the keywords of local_search as a dict (an empty one: its defaults).  The kept hits are then refined by
        local_search and ordered by their refined score (stable for ties), the LocalHit list is returned, and the filter is
        initialised at the best one's mean_pose with its cov + diag(step_xy^2, step_xy^2, step_theta^2) / 12 - the variance of a
        uniform error inside one lattice step, which keeps the matrix positive definite on a plateau or with no steps at all.  Where
        the best hit's moments are not valid the caller's covariance is used; `covariance` may be None only with refine."""
        if refine is None and covariance is None:
            raise ValueError("relocalize: a covariance is needed unless refine is given")
        hits = self.global_search(measurement, **search)
        if refine is None:
            if hits:
                best = hits[0]
                self.initialize([best.pose[2], best.pose[3], math.atan2(best.pose[1], best.pose[0])], covariance)
            return hits
        if not hits:
            return []
        refined = self.local_search(np.array([h.pose for h in hits]), measurement, **refine)
        refined.sort(key=lambda h: -h.score)  # (sort is stable: equal scores keep the search's order)
        best = refined[0]
        step_xy, step_theta = self.last_local_search_info["step_xy"], self.last_local_search_info["step_theta"]
        if best.moments_valid:
            cov = best.cov + np.diag([step_xy * step_xy / 12.0, step_xy * step_xy / 12.0, step_theta * step_theta / 12.0])
        elif covariance is None:
            raise ValueError("relocalize: the best hit's moments are not valid and no covariance was given")
        else:
            cov = covariance
        self.initialize([best.mean_pose[2], best.mean_pose[3], math.atan2(best.mean_pose[1], best.mean_pose[0])], cov)
        return refined

    # -- local pose search: a lattice of offsets about each seed pose, its best and the response's moments (mcl_local_search*) -------
    def _local_params(self, half_steps_xy, half_steps_theta, step_xy, step_theta):
        return capi.LocalSearchParams(int(half_steps_xy), int(half_steps_theta), 0.0 if step_xy is None else float(step_xy), float(step_theta))

    def local_search(self, poses, measurement, half_steps_xy=4, half_steps_theta=5, step_xy=None, step_theta=math.pi / 360):
        """The correlative scan matcher about each of `poses` (float64 (n, 4) as (cos, sin, x, y)): the lattice of
        (2 half_steps_xy + 1)^2 (2 half_steps_theta + 1) poses at offsets of step_xy (None: a quarter of the map's cell size) in world x
        and y and of step_theta in heading is scored on the device as likelihoods() would score it.  Per seed a LocalHit: the best
        lattice pose (ties go to the one nearest the seed), its score, the seed's own, and the score-weighted mean pose and covariance
        of the lattice.  The filter is untouched.  Every sensor model; the measurement as likelihoods() takes it.
        last_local_search_info holds the call's counts and steps."""
        p = _f64_rows("poses", poses, 4)
        params = self._local_params(half_steps_xy, half_steps_theta, step_xy, step_theta)
        hits = (capi.LocalHit * max(len(p), 1))()
        info = capi.LocalSearchInfo()
        if self._landmark_kind:
            landmark = self._landmark_kind == capi.MCL_SENSOR_LANDMARK
            xyz, cat = _likelihood_detections(measurement, "detection_position_in_robot" if landmark else "detection_bearing_in_sensor")
            fn = self._lib.mcl_local_search_landmarks if landmark else self._lib.mcl_local_search_bearings
            self._check(fn(self._ctx, _dp(p), len(p), _dp(xyz), cat.ctypes.data_as(capi.c_u32_p), len(xyz), C.byref(params), hits, C.byref(info)))
        else:
            pts = _f64_rows("points", measurement, 2)
            self._check(self._lib.mcl_local_search(self._ctx, _dp(p), len(p), _dp(pts), len(pts), C.byref(params), hits, C.byref(info)))
        self.last_local_search_info = {name: getattr(info, name) for name, _ in capi.LocalSearchInfo._fields_}
        self.last_local_search_info["step_theta"] = params.step_theta
        return [LocalHit(np.array(h.pose, dtype=np.float64), h.score, h.seed_score, h.di, h.dj, h.dk, h.plateau,
                         np.array(h.mean_pose, dtype=np.float64), np.array(h.cov, dtype=np.float64).reshape(3, 3),
                         np.array(h.sums, dtype=np.float64), bool(h.moments_valid)) for h in hits[:len(p)]]

    def local_search_candidates(self, pose, half_steps_xy=4, half_steps_theta=5, step_xy=None, step_theta=math.pi / 360, first=0, count=None):
        """The lattice of one seed as the device makes it, in id order: (poses float64 (k, 4), total).  count None: all from `first` on."""
        seed = _f64_rows("pose", np.asarray(pose, dtype=np.float64).reshape(1, -1), 4)
        params = self._local_params(half_steps_xy, half_steps_theta, step_xy, step_theta)
        total = C.c_uint64(0)
        if count is None:
            self._check(self._lib.mcl_local_search_candidates(self._ctx, _dp(seed), C.byref(params), 0, 0, None, C.byref(total)))
            count = max(total.value - int(first), 0)
        poses = np.zeros((int(count), 4), dtype=np.float64)
        self._check(self._lib.mcl_local_search_candidates(self._ctx, _dp(seed), C.byref(params), int(first), int(count), _dp(poses), C.byref(total)))
        return poses[:min(int(count), max(total.value - int(first), 0))], total.value

    # -- beam skipping (Nav2's do_beamskip; likelihood-field filters) -------------------------------------------------------------
    def set_beam_skip(self, enabled: bool = True, distance: Optional[float] = None, threshold: Optional[float] = None,
                      error_threshold: Optional[float] = None):
        """mcl_set_beam_skip: before every reweight the cloud votes on each beam, and beams whose end-point lands within `distance` of
        an obstacle for no more than `threshold` of the particles are left out of that update - unless `error_threshold` of the scan
        or more would go, in which case all of it is used.  A value left None keeps what the filter has (Nav2's defaults at first:
        0.5 m, 0.3, 0.9)."""
        p = capi.BeamSkipParams()
        self._check(self._lib.mcl_get_beam_skip(self._ctx, C.byref(p)))
        p.enabled = int(bool(enabled))
        for name, value in (("distance", distance), ("threshold", threshold), ("error_threshold", error_threshold)):
            if value is not None:
                setattr(p, name, float(value))
        self._check(self._lib.mcl_set_beam_skip(self._ctx, C.byref(p)))

    def beam_skip(self) -> dict:
        """The parameters in force (mcl_get_beam_skip)."""
        p = capi.BeamSkipParams()
        self._check(self._lib.mcl_get_beam_skip(self._ctx, C.byref(p)))
        return {"enabled": bool(p.enabled), "distance": p.distance, "threshold": p.threshold, "error_threshold": p.error_threshold}

    def beam_skip_result(self) -> dict:
        """The decision of the last update or reweight with beam skipping on (mcl_get_beam_skip_result): valid, num_beams,
        num_particles, num_skipped, used_all, level, and per point of that call's scan `counts` (uint32) and `kept` (bool)."""
        r = capi.BeamSkipResult()
        self._check(self._lib.mcl_get_beam_skip_result(self._ctx, C.byref(r), None, None, 0))
        counts = np.zeros(r.num_beams if r.valid else 0, dtype=np.uint32)
        kept = np.zeros(len(counts), dtype=np.uint8)
        if len(counts):
            self._check(self._lib.mcl_get_beam_skip_result(self._ctx, C.byref(r), counts.ctypes.data_as(capi.c_u32_p),
                                                           kept.ctypes.data_as(C.POINTER(C.c_uint8)), len(counts)))
        return {"valid": bool(r.valid), "num_beams": r.num_beams, "num_particles": r.num_particles, "num_skipped": r.num_skipped,
                "used_all": bool(r.used_all), "level": r.level, "counts": counts, "kept": kept.astype(bool)}

    def beam_agreement(self, measurement) -> np.ndarray:
        """mcl_beam_agreement: for each point of `measurement` (float64 (B, 2), base frame) the number of particles of the current set
        whose end-point of it lands within the beam-skip distance of an obstacle - uint32 (B,).  The filter is untouched."""
        pts = _f64_rows("points", measurement, 2)
        counts = np.zeros(len(pts), dtype=np.uint32)
        self._check(self._lib.mcl_beam_agreement(self._ctx, _dp(pts), len(pts), counts.ctypes.data_as(capi.c_u32_p)))
        return counts

    def weight_sum(self) -> float:
        v = C.c_double(0)
        self._check(self._lib.mcl_weight_sum(self._ctx, C.byref(v)))
        return v.value

    def normalize(self, factor: float = float("nan")):
        st = capi.WeightStats()
        self._check(self._lib.mcl_normalize(self._ctx, factor, C.byref(st)))
        return {"sum": st.sum, "norm_sum": st.norm_sum, "norm_sumsq": st.norm_sumsq}

    def resample(self, random_state_probability: float, step: int) -> int:
        n = C.c_uint64(0)
        self._check(self._lib.mcl_resample(self._ctx, random_state_probability, step, C.byref(n)))
        return n.value

    def estimate_sums(self, pivot=(0.0, 0.0)) -> np.ndarray:
        p = np.ascontiguousarray(pivot, dtype=np.float64)
        out = np.zeros(12)
        self._check(self._lib.mcl_estimate_sums(self._ctx, _dp(p), _dp(out)))
        return out

    def estimate(self):
        est = capi.Estimate()
        self._check(self._lib.mcl_estimate_pose(self._ctx, C.byref(est)))
        return np.array(est.pose), np.array(est.covariance).reshape(3, 3)

    def cluster_based_estimate(self, linear_hash_resolution=0.20, angular_hash_resolution=0.524, weight_cap_percentile=0.90):
        """beluga::cluster_based_estimate (algorithm/cluster_based_estimation.hpp:415-433)."""
        cp = capi.ClusterParams(linear_hash_resolution, angular_hash_resolution, weight_cap_percentile)
        est = capi.Estimate()
        self._check(self._lib.mcl_cluster_based_estimate(self._ctx, C.byref(cp), C.byref(est)))
        return np.array(est.pose), np.array(est.covariance).reshape(3, 3)

    def estimate_clusters(self, linear_hash_resolution=0.20, angular_hash_resolution=0.524, weight_cap_percentile=0.90, max_clusters=64):
        """beluga::estimate_clusters (algorithm/cluster_based_estimation.hpp:337-399) over ParticleClusterizer's clusters: every
        hypothesis of the set, not the heaviest alone.  Returns (total, [(id, count, weight, mean, cov), ...]): how many clusters
        of more than one particle there are, and the heaviest min(max_clusters, 64, total) of them by descending weight (ties by
        ascending id); the first one is cluster_based_estimate's."""
        cp = capi.ClusterParams(linear_hash_resolution, angular_hash_resolution, weight_cap_percentile)
        capacity = max(0, min(int(max_clusters), capi.MCL_MAX_CLUSTER_ESTIMATES))
        out = (capi.ClusterEstimate * max(capacity, 1))()
        total = C.c_uint64(0)
        self._check(self._lib.mcl_estimate_clusters(self._ctx, C.byref(cp), out if capacity else None, capacity, C.byref(total)))
        found = [(int(e.id), int(e.count), float(e.weight), np.array(e.estimate.pose), np.array(e.estimate.covariance).reshape(3, 3))
                 for e in out[:min(capacity, total.value)]]
        return int(total.value), found

    def cluster_labels(self, linear_hash_resolution=0.20, angular_hash_resolution=0.524, weight_cap_percentile=0.90):
        """ParticleClusterizer::operator() (:269-304): the cluster id of every particle, in particles()' order (np.uint32[n])."""
        cp = capi.ClusterParams(linear_hash_resolution, angular_hash_resolution, weight_cap_percentile)
        n = C.c_uint64(0)
        self._check(self._lib.mcl_num_particles(self._ctx, C.byref(n)))
        labels = np.empty(n.value, dtype=np.uint32)
        self._check(self._lib.mcl_cluster_labels(self._ctx, C.byref(cp), labels.ctypes.data_as(capi.c_u32_p)))
        return labels

    def set_estimate_kind(self, cluster_based: bool, **cluster_params):
        """What update() returns: beluga::estimate (beluga::Amcl) or cluster_based_estimate (beluga_ros::Amcl).
        On a sharded filter (comm_attach_rccl) a COLLECTIVE call: every rank makes it, concurrently, with the same arguments."""
        cp = capi.ClusterParams(cluster_params.get("linear_hash_resolution", 0.20), cluster_params.get("angular_hash_resolution", 0.524),
                                cluster_params.get("weight_cap_percentile", 0.90))
        self._check(self._lib.mcl_set_estimate_kind(self._ctx, int(cluster_based), C.byref(cp)))

    def build_cdf(self) -> float:
        t = C.c_double(0)
        self._check(self._lib.mcl_build_cdf(self._ctx, C.byref(t)))
        return t.value

    def device_view(self) -> capi.DeviceView:
        v = capi.DeviceView()
        self._check(self._lib.mcl_get_device_view(self._ctx, C.byref(v)))
        return v

    def set_num_particles(self, n: int):
        self._check(self._lib.mcl_set_num_particles(self._ctx, n))

    def resample_targets(self, step: int, random_state_probability: float, total: float, first_slot: int, count: int, d_targets: int):
        self._check(self._lib.mcl_resample_targets(self._ctx, step, random_state_probability, total, first_slot, count, d_targets))

    def route_targets(self, d_targets, count, d_ends, d_offsets, world, self_rank, d_send, d_order, d_counts):
        self._check(self._lib.mcl_route_targets(self._ctx, d_targets, count, d_ends, d_offsets, world, self_rank, d_send, d_order, d_counts))

    def serve_requests(self, d_requests, m, d_replies):
        self._check(self._lib.mcl_serve_requests(self._ctx, d_requests, m, d_replies))

    def commit_routed(self, step, first_slot, count, d_replies, d_order, d_targets):
        self._check(self._lib.mcl_commit_routed(self._ctx, step, first_slot, count, d_replies, d_order, d_targets))

    def finish_candidates(self, step, first_slot, count, d_replies, d_order, d_targets, d_states, d_hashes):
        self._check(self._lib.mcl_finish_candidates(self._ctx, step, first_slot, count, d_replies, d_order, d_targets, d_states, d_hashes))

    def kld_begin(self):
        self._check(self._lib.mcl_kld_begin(self._ctx))

    def kld_feed(self, d_hashes: int, count: int):
        """-> global index of the first candidate failing kld_condition, or None if the whole block passes."""
        fail = C.c_uint64(0)
        self._check(self._lib.mcl_kld_feed(self._ctx, d_hashes, count, C.byref(fail)))
        return None if fail.value == 0xFFFFFFFFFFFFFFFF else int(fail.value)

    def load_shard(self, d_states: int, n: int, shard_offset: int):
        self._check(self._lib.mcl_load_shard(self._ctx, d_states, n, shard_offset))

    def weight_sum_device(self, d_sum: int):
        self._check(self._lib.mcl_weight_sum_device(self._ctx, d_sum))

    def normalize_device(self, d_factor: int, d_stats: int):
        self._check(self._lib.mcl_normalize_device(self._ctx, d_factor, d_stats))

    def build_cdf_device(self, d_total: int):
        self._check(self._lib.mcl_build_cdf_device(self._ctx, d_total))

    def estimate_sums_device(self, pivot, d_sums: int):
        p = np.ascontiguousarray(pivot, dtype=np.float64)
        self._check(self._lib.mcl_estimate_sums_device(self._ctx, _dp(p), d_sums))

    def sync(self):
        self._check(self._lib.mcl_sync(self._ctx))

    def beam_cells_visited(self, reset: bool = True) -> int:
        v = C.c_uint64(0)
        self._check(self._lib.mcl_beam_cells_visited(self._ctx, C.byref(v), int(reset)))
        return v.value

    # -- measurement hooks ---------------------------------------------------------------------------
    def profile_enable(self, on=True):
        """True / 2: HIP events around every stage; 1: around the sensor kernel only (what a timed run can afford: an event
        record costs ~5 us of stream time); False / 0: off."""
        level = 2 if on is True else int(on)
        self._check(self._lib.mcl_profile_enable(self._ctx, level))

    def comm_attach_rccl(self, unique_id: bytes, rank: int, world: int):
        """Joins the RCCL communicator of a sharded filter (include/beluga_mcl.h, "Particle shards"): this context must have been
        created with its shard_offset / shard_capacity; update() then runs the cycle over all shards.  COLLECTIVE for world > 1: the
        ranks attach concurrently (they exchange a word of their configuration and fail alike on a mismatch); set_option("device_policy")
        and set_estimate_kind are collective on an attached filter as well."""
        assert len(unique_id) == 128
        self._check(self._lib.mcl_comm_attach_rccl(self._ctx, unique_id, rank, world))

    def set_option(self, name: str, value: int):
        """A/B switch of the library (include/beluga_mcl.h, mcl_set_option); no option but field_build changes a result
        beyond the rounding of a particle's sum over the scan."""
        self._check(self._lib.mcl_set_option(self._ctx, name.encode(), int(value)))

    def debug_set_recovery_filters(self, slow: float, fast: float):
        """Test hook (mcl_debug_set_recovery_filters): the outputs of the recovery estimator's two exponential filters."""
        self._check(self._lib.mcl_debug_set_recovery_filters(self._ctx, float(slow), float(fast)))

    def last_sampler(self) -> np.ndarray:
        """Test hook (mcl_debug_last_sampler): the sampler the last propagation's kernel received, bit for bit -
        (m1, s1, mt, st, m2, s2, kind, first_c, first_s).  Raises before the first propagation."""
        out = np.zeros(9)
        self._check(self._lib.mcl_debug_last_sampler(self._ctx, _dp(out)))
        return out

    def counter(self, name: str) -> int:
        v = C.c_uint64(0)
        self._check(self._lib.mcl_get_counter(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def debug_order(self):
        """(perm, keys) of the spatial ordering of the current set: keys[perm] is non-decreasing."""
        n = self.num_particles()
        perm, keys = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._check(self._lib.mcl_debug_order(self._ctx, perm.ctypes.data_as(capi.c_u32_p), keys.ctypes.data_as(capi.c_u32_p)))
        return perm, keys

    def profile_read(self, reset: bool = True):
        ms = (C.c_double * len(capi.STAGES))()
        cnt = (C.c_uint64 * len(capi.STAGES))()
        self._check(self._lib.mcl_profile_read(self._ctx, ms, cnt, int(reset)))
        return {name: (ms[i], cnt[i]) for i, name in enumerate(capi.STAGES)}


class AmclBatch:
    """A fleet of small filters that share their launches (mcl_batch_*): one update call, three kernel launches for all members whose
    cycle is the small one, one synchronisation - and two more shared launches for those of them that return the cluster-based estimate.  specs: one entry per member, the argument set of Amcl(...) - a dict of keyword
    arguments, or a tuple of positional ones that may end with such a dict; `grid` may be None (the member gets its map later).
    Every member is on one device and one stream (`hip_stream`: all 0, or all the same).  members[i] are Amcl objects bound to the
    batch's contexts: every Amcl method works on them between batch updates; they do not own their contexts (close() does nothing)."""

    def __init__(self, specs):
        self._lib = capi.load()
        self.members = []
        grids, options, cfgs = [], [], (capi.Config * len(specs))()
        for i, spec in enumerate(specs):
            args, kwargs = (), {}
            if isinstance(spec, dict):
                kwargs = dict(spec)
            else:
                args = tuple(spec)
                if args and isinstance(args[-1], dict):
                    args, kwargs = args[:-1], dict(args[-1])
            names = ("grid", "motion", "sensor", "params")
            kwargs.update(zip(names, args))
            member = Amcl.__new__(Amcl)
            grids.append(kwargs.pop("grid", None))
            options.append(kwargs.pop("options", None))
            cfgs[i] = member._configure(grids[-1], kwargs.pop("motion"), kwargs.pop("sensor"), kwargs.pop("params", AmclParams()), **kwargs)
            self.members.append(member)
        self._batch = capi._batch()
        st = self._lib.mcl_batch_create(cfgs, len(specs), C.byref(self._batch))
        if st != capi.MCL_OK:
            self._batch = None
            for member in self.members:
                member._ctx = None
            raise capi.MclError(st, self._lib.mcl_batch_last_error(None).decode())
        n = len(self.members)
        for i, member in enumerate(self.members):
            ctx = capi._ctx()
            self._check(self._lib.mcl_batch_member(self._batch, i, C.byref(ctx)))
            member._attach(ctx, grids[i], options[i], owned=False)
        self._controls = np.zeros((n, 4), dtype=np.float64)
        self._offsets = np.zeros(n + 1, dtype=np.uint64)
        self._estimates = (capi.Estimate * n)()
        self._infos = (capi.UpdateInfo * n)()
        self._statuses = (C.c_int32 * n)()
        self._est_view = np.frombuffer(self._estimates, dtype=np.float64).reshape(n, 13)
        self._have_info = False
        self.last_status = capi.MCL_OK

    def close(self):
        if getattr(self, "_batch", None):
            self._lib.mcl_batch_destroy(self._batch)
            self._batch = None
            for member in self.members:
                member._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.members)

    def _check(self, st):
        if st != capi.MCL_OK:
            raise capi.MclError(st, self._lib.mcl_batch_last_error(self._batch).decode())

    def update(self, control_actions, measurements, check: bool = True):
        """Amcl::update on every member: control_actions[i] and measurements[i] (points[n_i, 2]) are member i's.  Returns a list with
        (pose, covariance) or None per member, bit for bit what members[i].update(...) returns.  check = False: a member's failure does
        not raise; its entry is None and `statuses` / `last_status` tell."""
        n = len(self.members)
        if len(control_actions) != n or len(measurements) != n:
            raise ValueError("AmclBatch.update: one control action and one measurement per member")
        for i in range(n):
            self._controls[i] = control_actions[i]
        scans = [np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 2) for m in measurements]
        self._offsets[1:] = np.cumsum([len(m) for m in scans])
        points = np.concatenate(scans) if n else np.zeros((0, 2))
        points = np.ascontiguousarray(points, dtype=np.float64)
        self.last_status = self._lib.mcl_batch_update(self._batch, _dp(self._controls), _dp(points), self._offsets.ctypes.data_as(capi.c_u64_p),
                                                      self._estimates, self._infos, self._statuses)
        self._have_info = True
        if check:
            self._check(self.last_status)
        return self._results()

    def _results(self):
        """(pose, covariance) or None per member, from what the last call left."""
        out = []
        for i in range(len(self.members)):
            if self._statuses[i] != capi.MCL_OK or not self._infos[i].updated:
                out.append(None)
                continue
            e = self._est_view[i].copy()
            out.append((e[:4], e[4:13].reshape(3, 3)))
        return out

    def update_detections(self, controls, detections_per_member, check: bool = True):
        """Amcl::update on every member of a fleet of landmark and bearing filters (mcl_landmark_batch_update): controls[i] and
        detections_per_member[i] - a list of LandmarkPositionDetection / LandmarkBearingDetection or a (vectors, categories) pair -
        are member i's.  Returns what update returns: (pose, covariance) or None per member, bit for bit members[i].update(...)'s.
        Members with set_landmark_small_cycle(True) share three launches; the others run their own cycle inside the call."""
        n = len(self.members)
        if len(controls) != n or len(detections_per_member) != n:
            raise ValueError("AmclBatch.update_detections: one control action and one list of detections per member")
        vectors, categories = [], []
        for i, member in enumerate(self.members):
            self._controls[i] = controls[i]
            attribute = "detection_bearing_in_sensor" if member._landmark_kind == capi.MCL_SENSOR_BEARING else "detection_position_in_robot"
            xyz, cat = _detection_arrays(detections_per_member[i], attribute)
            vectors.append(xyz)
            categories.append(cat)
        self._offsets[1:] = np.cumsum([len(v) for v in vectors])
        return self.update_detection_offsets(self._controls, np.concatenate(vectors) if n else np.zeros((0, 3)),
                                             np.concatenate(categories) if n else np.zeros(0, dtype=np.uint32), self._offsets, check=check)

    def update_detection_offsets(self, controls, vectors_xyz, categories, detection_offsets, check: bool = False):
        """The C call as it is: all detections in one vectors_xyz[total, 3] and categories[total] with detection_offsets[n + 1].
        Returns the members' results; `last_status` and `statuses` tell what the call and every member answered."""
        ctrl = np.ascontiguousarray(controls, dtype=np.float64).reshape(len(self.members), 4)
        xyz = np.ascontiguousarray(vectors_xyz, dtype=np.float64)
        cat = np.ascontiguousarray(categories, dtype=np.uint32)
        off = np.ascontiguousarray(detection_offsets, dtype=np.uint64)
        self.last_status = self._lib.mcl_landmark_batch_update(self._batch, _dp(ctrl), _dp(xyz), cat.ctypes.data_as(capi.c_u32_p),
                                                               off.ctypes.data_as(capi.c_u64_p), self._estimates, self._infos, self._statuses)
        self._have_info = True
        if check:
            self._check(self.last_status)
        return self._results()

    def update_offsets(self, control_actions, points_xy, point_offsets):
        """The C call as it is: all scans in one points_xy[total, 2] with point_offsets[n + 1]; returns the call's status."""
        ctrl = np.ascontiguousarray(control_actions, dtype=np.float64).reshape(len(self.members), 4)
        pts = np.ascontiguousarray(points_xy, dtype=np.float64)
        off = np.ascontiguousarray(point_offsets, dtype=np.uint64)
        self.last_status = self._lib.mcl_batch_update(self._batch, _dp(ctrl), _dp(pts), off.ctypes.data_as(capi.c_u64_p), self._estimates,
                                                      self._infos, self._statuses)
        self._have_info = True
        return self.last_status

    @property
    def statuses(self):
        """Every member's status of the last update."""
        return [int(s) for s in self._statuses]

    @property
    def last_infos(self):
        """mcl_update_info of every member's last batch update, as Amcl.last_info's dicts (None before the first update)."""
        if not self._have_info:
            return None
        return [{"updated": bool(info.updated), "resampled": bool(info.resampled), "num_particles": info.num_particles,
                 "weight_sum": info.weight_sum, "ess": info.effective_sample_size,
                 "random_state_probability": info.random_state_probability} for info in self._infos]

    def set_option(self, name: str, value: int):
        """mcl_set_option on every member, e.g. batch_cluster_fused (default 1; 0: the member's cluster-based estimate through its own
        kernels instead of the fleet's two shared launches)."""
        for member in self.members:
            member.set_option(name, value)

    def ndt_counts(self) -> Tuple[int, int]:
        """(shared NDT reweight launches enqueued, NDT members that updated through the shared launches): running totals
        (mcl_ndt_batch_counts)."""
        launches, members = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.mcl_ndt_batch_counts(self._batch, C.byref(launches), C.byref(members)))
        return launches.value, members.value

    def counter(self, name: str) -> int:
        """cycles, kernel_launches, members_fused, members_alone, cluster_launches, members_cluster_fused, cluster_host_ns, beam_launches,
        members_beam_fused, landmark_launches, members_landmark_fused (mcl_batch_get_counter)."""
        value = C.c_uint64(0)
        self._check(self._lib.mcl_batch_get_counter(self._batch, name.encode(), C.byref(value)))
        return value.value


def make_laser_scan(ranges, angle_min, angle_increment, range_min, range_max, origin_se3=(0, 0, 0, 1, 0, 0, 0), max_beams=2 ** 64 - 1,
                    min_range=float(np.finfo(np.float64).tiny), max_range=float(np.finfo(np.float64).max)):
    """A beluga_ros::LaserScan (laser_scan.hpp:46-66): the message fields + origin + decimation / range limits."""
    r = np.ascontiguousarray(ranges, dtype=np.float32)
    scan = capi.LaserScan()
    scan.ranges = r.ctypes.data_as(capi.c_float_p)
    scan.num_ranges = len(r)
    scan.angle_min, scan.angle_increment = angle_min, angle_increment
    scan.range_min, scan.range_max = range_min, range_max
    scan.origin_se3 = (C.c_double * 7)(*origin_se3)
    scan.max_beams = max_beams
    scan.min_range, scan.max_range = min_range, max_range
    scan._keepalive = r
    return scan


def prepare_laser_scan(scan) -> np.ndarray:
    """points in the base frame, as beluga_ros::Amcl::update builds them (beluga_ros/src/amcl.cpp:54-63)."""
    lib = capi.load()
    out = np.zeros((min(scan.num_ranges, scan.max_beams) + 1, 2))
    m = C.c_uint64(0)
    st = lib.mcl_prepare_laser_scan(C.byref(scan), _dp(out), C.byref(m))
    if st != capi.MCL_OK:
        raise capi.MclError(st, "mcl_prepare_laser_scan")
    return out[:m.value].copy()


def estimate_from_sums(sums: np.ndarray):
    lib = capi.load()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    est = capi.Estimate()
    st = lib.mcl_estimate_from_sums(_dp(s), C.byref(est))
    if st != capi.MCL_OK:
        raise capi.MclError(st, "mcl_estimate_from_sums")
    return np.array(est.pose), np.array(est.covariance).reshape(3, 3)


def project_point_cloud(points_xyz, origin_se3=(0, 0, 0, 1, 0, 0, 0)) -> np.ndarray:
    """Points of a beluga_ros::SparsePointCloud3f in the base frame, projected onto z = 0 (beluga_ros/src/amcl.cpp:73-76)."""
    lib = capi.load()
    pts = np.ascontiguousarray(points_xyz, dtype=np.float32).reshape(-1, 3)
    origin = np.ascontiguousarray(origin_se3, dtype=np.float64)
    out = np.zeros((len(pts), 2))
    st = lib.mcl_project_point_cloud(pts.ctypes.data_as(capi.c_float_p), len(pts), _dp(origin), _dp(out))
    if st != capi.MCL_OK:
        raise capi.MclError(st, "mcl_project_point_cloud")
    return out


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls it and hands the 128 bytes to the other ranks)."""
    lib = capi.load()
    buf = C.create_string_buffer(128)
    st = lib.mcl_comm_unique_id(buf)
    if st != capi.MCL_OK:
        raise capi.MclError(st, lib.mcl_last_error(None).decode())
    return buf.raw
