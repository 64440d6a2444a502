"""Host-side mirror of the reference's registration interfaces for the hot path.

  ICP                          <-> PointMatcher<float>::ICP   (libpointmatcher/pointmatcher/PointMatcher.h:1023-1060,
                                   ICP.cpp:793-898; configured like ICPChainBase::setDefault / loadFromYaml,
                                   ICP.cpp:100-210), as used by o3d_slam::Mapper (Mapper.cpp:343,372-373)
  RegistrationIcpGeneralized   <-> o3d_slam::RegistrationIcpGeneralized::registerClouds
                                   (open3d_slam/src/CloudRegistration.cpp:16-21, CloudRegistration.hpp:19-73)
  RegistrationIcpPointToPlane  <-> o3d_slam::RegistrationIcpPointToPlane (CloudRegistration.cpp:54-83)
  RegistrationIcpPointToPoint  <-> o3d_slam::RegistrationIcpPointToPoint (CloudRegistration.cpp:84-101)
  cloudRegistrationFactory     <-> o3d_slam::cloudRegistrationFactory (CloudRegistration.cpp:104-119)

Same method names, argument meaning and error behaviour (exceptions named after the reference's);
all compute goes through the C ABI (capi.Registration) to the HIP kernels -- nothing is computed here.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from . import capi
from .capi import RegError, RegParams


class ConvergenceError(RuntimeError):
    """PointMatcher<T>::ConvergenceError (ErrorMinimizer.cpp:75-77, Matches.cpp:76-80)."""


class InvalidField(RuntimeError):
    """DataPoints::InvalidField (DataPoints.cpp:1112)."""


class InvalidModuleType(RuntimeError):
    """PointMatcherSupport::InvalidModuleType (ICP.cpp:203-209)."""


class InvalidParameter(RuntimeError):
    """Parametrizable::InvalidParameter (Registrar.h:103-109)."""


@dataclass
class DataPoints:
    """The fields of PointMatcher<float>::DataPoints the path touches (PointMatcher.h:222-403):
    `features` N x 4 ({x,y,z,1} per point == the column-major 4 x N Eigen matrix in memory) or N x 3,
    descriptor `normals` N x 3."""
    features: np.ndarray
    normals: np.ndarray | None = None
    covariances: np.ndarray | None = None

    def getNbPoints(self) -> int:
        return 0 if self.features is None else int(np.asarray(self.features).shape[0])


def _translate(e: RegError):
    if e.status == 3:
        return ConvergenceError(str(e))
    if e.status == 7:
        return InvalidField(str(e))
    if e.status == 6:
        return InvalidParameter(str(e))
    return RuntimeError(str(e))


_KNOWN_TOP = {"readingDataPointsFilters", "referenceDataPointsFilters", "readingStepDataPointsFilters", "matcher",
              "outlierFilters", "errorMinimizer", "transformationCheckers", "inspector", "logger",
              "degeneracyDebug", "printingDegeneracy", "ceresDegeneracyAnalysis", "degeneracyAwareness"}


class ICP:
    """Drop-in for the `icp_` member of o3d_slam::Mapper: initReference() once per map refresh,
    compute() per scan."""

    def __init__(self):
        self.params: RegParams | None = None
        self._reg: capi.Registration | None = None
        self.matcherIsInitialized = False
        self.maxNumIterationsReached = False
        self.last_result = None

    # -- configuration --------------------------------------------------------------------------
    def setDefault(self):
        """ICPChainBase::setDefault (ICP.cpp:100-113)."""
        self.params = capi.default_params()
        self._reg = None
        self.matcherIsInitialized = False

    def loadFromYaml(self, stream_or_text):
        """The hot-path subset of ICPChainBase::loadFromYaml (ICP.cpp:116-210)."""
        import yaml
        text = stream_or_text.read() if hasattr(stream_or_text, "read") else stream_or_text
        doc = yaml.safe_load(text) or {}
        for key in doc:
            if key not in _KNOWN_TOP:
                raise InvalidModuleType(f"Module type {key} does not exist")
        p = capi.default_params()
        p.use_trimmed = 0
        p.max_iter = 1 << 30
        p.smooth_len = 0
        for name in ("readingDataPointsFilters", "referenceDataPointsFilters", "readingStepDataPointsFilters"):
            if doc.get(name):
                raise NotImplementedError(f"{name}: data-point filters are outside the accelerated path "
                                          "(the shipped icp.yaml leaves these chains empty)")
        m = doc.get("matcher")
        if m:
            (mname, margs), = (m.items() if isinstance(m, dict) else [(m, {})])
            if mname != "KDTreeMatcher":
                raise NotImplementedError(f"matcher {mname}")
            margs = margs or {}
            p.knn = int(margs.get("knn", 1))
            p.max_dist = float(margs.get("maxDist", math.inf))
            p.epsilon = float(margs.get("epsilon", 0.0))
        for f in doc.get("outlierFilters") or []:
            (fname, fargs), = (f.items() if isinstance(f, dict) else [(f, {})])
            fargs = fargs or {}
            if fname == "TrimmedDistOutlierFilter":
                p.use_trimmed, p.trim_ratio = 1, float(fargs.get("ratio", 0.85))
            elif fname == "SurfaceNormalOutlierFilter":
                p.use_surface_normal, p.max_normal_angle = 1, float(fargs.get("maxAngle", 1.57))
            elif fname == "MaxDistOutlierFilter":
                p.use_max_dist_filter, p.outlier_max_dist = 1, float(fargs.get("maxDist", 1.0))
            elif fname == "NullOutlierFilter":
                pass
            else:
                raise NotImplementedError(f"outlier filter {fname}")
        em = doc.get("errorMinimizer", "PointToPlaneErrorMinimizer")
        emname = next(iter(em)) if isinstance(em, dict) else em
        if emname != "PointToPlaneErrorMinimizer":
            raise NotImplementedError(f"errorMinimizer {emname}")
        for c in doc.get("transformationCheckers") or []:
            (cname, cargs), = (c.items() if isinstance(c, dict) else [(c, {})])
            cargs = cargs or {}
            if cname == "CounterTransformationChecker":
                p.max_iter = int(cargs.get("maxIterationCount", 40))
            elif cname == "DifferentialTransformationChecker":
                p.min_diff_rot = float(cargs.get("minDiffRotErr", 0.001))
                p.min_diff_trans = float(cargs.get("minDiffTransErr", 0.001))
                p.smooth_len = int(cargs.get("smoothLength", 3))
            else:
                raise NotImplementedError(f"transformation checker {cname}")
        da = doc.get("degeneracyAwareness")
        if da:
            # ICPChainBase::loadAdditionalYAMLContent (ICP.cpp:575-790): only the shipped method is accelerated
            (dname, dargs), = (da.items() if isinstance(da, dict) else [(da, {})])
            dargs = dargs or {}
            if dname == "OptimizedEqualityConstraints":
                need = ("enoughInformationThreshold", "insufficientInformationThreshold",
                        "point2NormalMinimalAlignmentAngleThreshold", "point2NormalStrongAlignmentAngleThreshold")
                if any(k not in dargs for k in need):
                    raise InvalidParameter("OptimizedEqualityConstraints needs " + ", ".join(need))   # ICP.cpp:632-672
                p.use_xicp = 1
                p.xicp_enough = float(dargs[need[0]])
                p.xicp_insufficient = float(dargs[need[1]])
                p.xicp_min_angle_deg = float(dargs[need[2]])
                p.xicp_strong_angle_deg = float(dargs[need[3]])
            elif dname in ("None", "none", "kNone"):
                pass
            else:
                raise NotImplementedError(f"degeneracyAwareness method {dname}")
        if p.knn != 1:
            raise InvalidParameter("knn must be 1 on the accelerated path")
        self.params = p
        self._reg = None
        self.matcherIsInitialized = False

    # -- the two calls Mapper makes ----------------------------------------------------------------
    def _ensure(self):
        if self.params is None:
            raise RuntimeError("You must setup a matcher before running ICP")  # ICP.cpp:819-824
        if self._reg is None:
            self._reg = capi.Registration(self.params)

    def hasMap(self) -> bool:
        return self.matcherIsInitialized

    def initReference(self, referenceIn: DataPoints) -> bool:
        """ICP::initReference (ICP.cpp:847-898).  Returns False on an empty reference."""
        self._ensure()
        if referenceIn.getNbPoints() == 0:
            print("The reference point cloud is empty. (libpointmatcher)")
            self.matcherIsInitialized = False
            return False
        try:
            self._reg.set_target(referenceIn.features, referenceIn.normals, referenceIn.covariances)
        except RegError as e:
            raise _translate(e) from None
        self.matcherIsInitialized = True
        return True

    def compute(self, readingIn: DataPoints, referenceIn: DataPoints | None = None, T_refIn_readIn=None,
                initializeMatcherWithInputReference: bool = True) -> np.ndarray:
        """ICP::compute (ICP.cpp:813-844)."""
        self._ensure()
        if initializeMatcherWithInputReference or not self.matcherIsInitialized:
            if referenceIn is None or not self.initReference(referenceIn):
                return np.eye(4, dtype=np.float32)
        T = np.eye(4, dtype=np.float32) if T_refIn_readIn is None else np.asarray(T_refIn_readIn, np.float32)
        if T.shape != (4, 4):
            raise RuntimeError("The initial transformation matrix must be squared.")  # ICP.cpp:910-918
        if readingIn.getNbPoints() == 0:
            raise RuntimeError("The reading point cloud is empty.")  # ICP.cpp:958-960
        try:
            self._reg.set_source(readingIn.features, readingIn.normals, readingIn.covariances)
            T_out, res = self._reg.register(T)
        except RegError as e:
            raise _translate(e) from None
        self.last_result = res
        self.maxNumIterationsReached = bool(res.max_iter_reached)
        return T_out

    def __call__(self, readingIn, referenceIn, T_refIn_readIn=None):
        return self.compute(readingIn, referenceIn, T_refIn_readIn, True)


class PointMatcherICP(ICP):
    """ICP with the libpointmatcher chain extension (include/o3dslam_reg.h, reg_set_pm_chain): loadFromYaml also takes
    KDTreeMatcher.knn up to 16, RobustOutlierFilter (OutlierFiltersImpl.h:230-244 names and defaults) and
    PointToPointErrorMinimizer; everything else binds exactly as for ICP.  The filter's scale / iteration persist
    across compute() calls on the same object, as in the reference."""

    _ROBUST_DEFAULTS = {"robustFct": "cauchy", "tuning": 1.0, "scaleEstimator": "mad", "nbIterationForScale": 0,
                        "distanceType": "point2point", "approximation": math.inf}

    def __init__(self):
        super().__init__()
        self.chain: capi.PmChain | None = None

    def setDefault(self):
        super().setDefault()
        self.chain = None

    def loadFromYaml(self, stream_or_text):
        import yaml
        text = stream_or_text.read() if hasattr(stream_or_text, "read") else stream_or_text
        doc = yaml.safe_load(text) or {}
        chain = capi.default_pm_chain()
        m = doc.get("matcher")
        if isinstance(m, dict) and isinstance(m.get("KDTreeMatcher"), dict) and "knn" in m["KDTreeMatcher"]:
            chain.knn = int(m["KDTreeMatcher"]["knn"])
            m["KDTreeMatcher"] = dict(m["KDTreeMatcher"], knn=1)
        kept = []
        for f in doc.get("outlierFilters") or []:
            (fname, fargs), = (f.items() if isinstance(f, dict) else [(f, {})])
            if fname != "RobustOutlierFilter":
                kept.append(f)
                continue
            if chain.use_robust:
                raise NotImplementedError("more than one RobustOutlierFilter")
            a = dict(self._ROBUST_DEFAULTS, **(fargs or {}))
            unknown = set(a) - set(self._ROBUST_DEFAULTS)
            if unknown:
                raise InvalidParameter(f"RobustOutlierFilter: unknown parameter(s) {sorted(unknown)}")
            if a["robustFct"] not in capi.ROBUST_FCTS:
                raise InvalidParameter("Invalid robust function name.")
            if a["scaleEstimator"] not in capi.SCALE_ESTIMATORS:
                raise InvalidParameter("Invalid scale estimator name.")
            if a["distanceType"] not in capi.DISTANCE_TYPES:
                raise InvalidParameter("Invalid distance type name.")
            chain.use_robust = 1
            chain.robust_fct = capi.ROBUST_FCTS[a["robustFct"]]
            chain.tuning = float(a["tuning"])
            chain.scale_estimator = capi.SCALE_ESTIMATORS[a["scaleEstimator"]]
            chain.nb_iter_for_scale = int(a["nbIterationForScale"])
            chain.distance_type = capi.DISTANCE_TYPES[a["distanceType"]]
            chain.approximation = float(a["approximation"])
        if "outlierFilters" in doc:
            doc["outlierFilters"] = kept
        em = doc.get("errorMinimizer", "PointToPlaneErrorMinimizer")
        if (next(iter(em)) if isinstance(em, dict) else em) == "PointToPointErrorMinimizer":
            chain.minimizer = capi.PM_POINT_TO_POINT
            doc["errorMinimizer"] = "PointToPlaneErrorMinimizer"
        super().loadFromYaml(yaml.safe_dump(doc))
        st = capi.check_pm_chain(self.params, chain)
        if st == 9:
            raise NotImplementedError("this chain is outside the accelerated path (std scale estimator, or X-ICP with "
                                      "k-NN / robust weights / point-to-point)")
        if st != 0:
            raise InvalidParameter("invalid chain (knn must lie in 1..16; robust parameters out of range)")
        self.chain = chain

    def _ensure(self):
        fresh = self._reg is None
        super()._ensure()
        if fresh and self.chain is not None:
            try:
                self._reg.set_pm_chain(self.chain)
            except RegError as e:
                raise _translate(e) from None


@dataclass
class SurfaceNormalDataPointsFilter:
    """SurfaceNormalDataPointsFilter (DataPointsFilters/SurfaceNormal.h:68-78, SurfaceNormal.cpp:152-252) on the
    device: parameters by the reference's names; `epsilon` must be 0 (the search is exact).  `filter` returns a
    DataPoints with the `normals` descriptor added (keepNormals) and keeps `eigValues` / `matchedIds` on the filter."""

    def __init__(self, knn=5, maxDist=float("inf"), epsilon=0.0, keepNormals=True, keepDensities=False,
                 keepEigenValues=False, keepEigenVectors=False, keepMatchedIds=False, keepMeanDist=False, viewpoint=None,
                 smoothNormals=False):
        if knn < 3:
            raise InvalidParameter("knn: minimum 3 (SurfaceNormal.h:68)")
        if knn > 32:
            raise InvalidParameter("knn: this build supports at most 32 neighbours")
        if epsilon != 0.0:
            raise InvalidParameter("epsilon: only the exact search (0) is implemented")
        if not (maxDist > 0):
            raise InvalidParameter("maxDist: must be > 0")
        self.knn, self.maxDist, self.keepNormals = int(knn), float(maxDist), keepNormals
        self.keepEigenValues, self.keepMatchedIds, self.viewpoint = keepEigenValues, keepMatchedIds, viewpoint
        self.keepDensities, self.keepEigenVectors, self.keepMeanDist = keepDensities, keepEigenVectors, keepMeanDist
        self.eigValues = self.matchedIds = self.densities = self.eigVectors = self.meanDists = None
        self.smoothNormals = bool(smoothNormals)   # SurfaceNormal.cpp:259-283 (in place, index order)
        self._reg = None

    def filter(self, cloud: DataPoints) -> DataPoints:
        if self._reg is None:
            self._reg = capi.Registration(capi.default_params())
        try:
            out = self._reg.estimate_normals(cloud.features, k=self.knn, max_dist=self.maxDist, viewpoint=self.viewpoint,
                                             want_eigvals=self.keepEigenValues, want_ids=self.keepMatchedIds or self.smoothNormals,
                                             want_densities=self.keepDensities, want_eigvecs=self.keepEigenVectors,
                                             want_mean_dists=self.keepMeanDist)
            if self.smoothNormals:
                out["normals"], _ = self._reg.smooth_normals(out["normals"], out["ids"])
        except RegError as e:
            raise _translate(e) from None
        self.eigValues, self.matchedIds = out.get("eigvals"), (out.get("ids") if self.keepMatchedIds else None)
        self.densities, self.eigVectors, self.meanDists = out.get("densities"), out.get("eigvecs"), out.get("mean_dists")
        return DataPoints(cloud.features, out["normals"] if self.keepNormals else cloud.normals, cloud.covariances)


@dataclass
class RegistrationResult:
    """open3d::pipelines::registration::RegistrationResult fields consumed by the reference
    (Odometry.cpp:56,77, PlaceRecognition.cpp:118)."""
    transformation_: np.ndarray = field(default_factory=lambda: np.eye(4))
    fitness_: float = 0.0
    inlier_rmse_: float = 0.0
    correspondence_set_: np.ndarray | None = None


class RegistrationIcpGeneralized:
    """o3d_slam::RegistrationIcpGeneralized (CloudRegistration.hpp:59-68, CloudRegistration.cpp:16-21)."""

    def __init__(self, maxCorrespondenceDistance_=1.0, max_iteration_=30):
        self.maxCorrespondenceDistance_ = maxCorrespondenceDistance_
        self.max_iteration_ = max_iteration_
        self.relative_fitness_ = 1e-6   # open3d::pipelines::registration::ICPConvergenceCriteria defaults
        self.relative_rmse_ = 1e-6
        self._reg = None

    def registerClouds(self, source: DataPoints, target: DataPoints, init=None) -> RegistrationResult:
        p = capi.default_params()
        p.cost = capi.COST_GICP
        p.use_trimmed = 0
        p.max_dist = self.maxCorrespondenceDistance_
        p.max_iter = self.max_iteration_
        # icpConvergenceCriteria_: only max_iteration_ is configured (CloudRegistration.cpp:45-52), so Open3D's defaults
        # relative_fitness_ = relative_rmse_ = 1e-6 end the loop
        p.gicp_stop_rule = 1
        p.gicp_rel_fitness = self.relative_fitness_
        p.gicp_rel_rmse = self.relative_rmse_
        reg = capi.Registration(p)
        try:
            reg.set_target(target.features, None, target.covariances)
            reg.set_source(source.features, None, source.covariances)
            T, res = reg.register(np.eye(4) if init is None else init)
            ids, _, _ = reg.correspondences(want_w=False)
        except RegError as e:
            raise _translate(e) from None
        finally:
            pass
        sel = np.nonzero(ids >= 0)[0]
        out = RegistrationResult(T.astype(np.float64), float(res.fitness), float(res.inlier_rmse),
                                 np.stack([sel, ids[sel]], axis=1))
        reg.close()
        return out


class _RegistrationIcpOpen3d:
    """Common part of the two Open3D RegistrationICP operators: the select-free iteration of the C ABI's
    REG_COST_O3D_P2PL / REG_COST_O3D_P2P, stopped by Open3D's ICPConvergenceCriteria (only max_iteration_ is configured,
    CloudRegistration.cpp:77-101, so relative_fitness_ = relative_rmse_ = 1e-6 end the loop)."""
    _cost = None
    _needs_target_normals = False

    def __init__(self, maxCorrespondenceDistance_=1.0, max_iteration_=30):
        self.maxCorrespondenceDistance_ = maxCorrespondenceDistance_
        self.max_iteration_ = max_iteration_
        self.relative_fitness_ = 1e-6   # open3d::pipelines::registration::ICPConvergenceCriteria defaults
        self.relative_rmse_ = 1e-6

    def params(self) -> RegParams:
        p = capi.default_params()
        p.cost = self._cost
        p.use_trimmed = 0
        p.max_dist = self.maxCorrespondenceDistance_
        p.max_iter = self.max_iteration_
        p.gicp_rel_fitness = self.relative_fitness_
        p.gicp_rel_rmse = self.relative_rmse_
        return p

    def registerClouds(self, source: DataPoints, target: DataPoints, init=None) -> RegistrationResult:
        if self._needs_target_normals and target.normals is None:
            # Open3D: "TransformationEstimationPointToPlane ... require pre-computed normal vectors for target PointCloud."
            raise InvalidField("point-to-plane needs normals on the target cloud")
        reg = capi.Registration(self.params())
        try:
            reg.set_target(target.features, target.normals if self._needs_target_normals else None, None)
            reg.set_source(source.features, None, None)
            T, res = reg.register(np.eye(4) if init is None else init)
            ids, _, _ = reg.correspondences(want_w=False)
        except RegError as e:
            raise _translate(e) from None
        finally:
            reg.close()
        sel = np.nonzero(ids >= 0)[0]
        return RegistrationResult(T.astype(np.float64), float(res.fitness), float(res.inlier_rmse),
                                  np.stack([sel, ids[sel]], axis=1))

    def estimateNormalsOrCovariancesIfNeeded(self, cloud: DataPoints) -> None:
        """Point-to-point needs neither normals nor covariances (CloudRegistration.hpp: the base class's no-op)."""


class RegistrationIcpPointToPlane(_RegistrationIcpOpen3d):
    """o3d_slam::RegistrationIcpPointToPlane (CloudRegistration.hpp:29-42, CloudRegistration.cpp:54-83): Open3D
    RegistrationICP with TransformationEstimationPointToPlane (L2 loss) -> REG_COST_O3D_P2PL."""
    _cost = capi.COST_O3D_P2PL
    _needs_target_normals = True

    def __init__(self, maxCorrespondenceDistance_=1.0, max_iteration_=30, knnNormalEstimation_=5,
                 maxRadiusNormalEstimation_=10.0):
        super().__init__(maxCorrespondenceDistance_, max_iteration_)
        self.knnNormalEstimation_ = knnNormalEstimation_
        self.maxRadiusNormalEstimation_ = maxRadiusNormalEstimation_

    def estimateNormalsOrCovariancesIfNeeded(self, cloud: DataPoints) -> None:
        """CloudRegistration.cpp:62-75: a cloud that has normals is left alone; otherwise k-NN normals within the radius,
        normalised and oriented towards the camera location (the origin) -- on the device (reg_estimate_normals)."""
        if cloud.normals is not None:
            return
        if not (self.maxRadiusNormalEstimation_ > 0.0):
            raise InvalidParameter("maxRadiusNormalEstimation_ must be > 0")
        if not (self.knnNormalEstimation_ > 0):
            raise InvalidParameter("knnNormalEstimation_ must be > 0")
        p = capi.default_params()
        p.cost = capi.COST_O3D_P2P
        reg = capi.Registration(p)
        try:
            out = reg.estimate_normals(cloud.features, k=self.knnNormalEstimation_, max_dist=self.maxRadiusNormalEstimation_,
                                       viewpoint=np.zeros(3, np.float32))
        except RegError as e:
            raise _translate(e) from None
        finally:
            reg.close()
        cloud.normals = out["normals"]


class RegistrationIcpPointToPoint(_RegistrationIcpOpen3d):
    """o3d_slam::RegistrationIcpPointToPoint (CloudRegistration.hpp:44-53, CloudRegistration.cpp:84-101): Open3D
    RegistrationICP with TransformationEstimationPointToPoint(with_scaling = false) -> REG_COST_O3D_P2P."""
    _cost = capi.COST_O3D_P2P


# CloudRegistrationType / ScanToMapRegistrationType (Parameters.hpp:37-49): same order, same strings
CLOUD_REGISTRATION_TYPES = {"PointToPlaneIcp": 0, "PointToPointIcp": 1, "GeneralizedIcp": 2}


def cloudRegistrationFactory(name_or_enum, maxCorrespondenceDistance_=0.2, maxNumIter_=50, knn_=5, maxDistanceKnn_=10.0):
    """o3d_slam::cloudRegistrationFactory (CloudRegistration.cpp:104-119) with the fields of IcpParameters
    (Parameters.hpp:66-72, defaults included): `cloud_registration_type` / `scan_to_map_refinement_type` string or the
    enum value."""
    kind = CLOUD_REGISTRATION_TYPES.get(name_or_enum) if isinstance(name_or_enum, str) else name_or_enum
    if kind == 0 and not isinstance(kind, bool):
        return RegistrationIcpPointToPlane(maxCorrespondenceDistance_, maxNumIter_, knn_, maxDistanceKnn_)
    if kind == 1 and not isinstance(kind, bool):
        return RegistrationIcpPointToPoint(maxCorrespondenceDistance_, maxNumIter_)
    if kind == 2 and not isinstance(kind, bool):
        return RegistrationIcpGeneralized(maxCorrespondenceDistance_, maxNumIter_)
    raise RuntimeError("cloud: unknown type of cloud registration")
