"""Host-side mirror of the reference's registration interfaces for the hot path.

  ICP                          <-> PointMatcher<float>::ICP   (libpointmatcher/pointmatcher/PointMatcher.h:1023-1060,
                                   ICP.cpp:793-898; configured like ICPChainBase::setDefault / loadFromYaml,
                                   ICP.cpp:100-210), as used by o3d_slam::Mapper (Mapper.cpp:343,372-373)
  RegistrationIcpGeneralized   <-> o3d_slam::RegistrationIcpGeneralized::registerClouds
                                   (open3d_slam/src/CloudRegistration.cpp:16-21, CloudRegistration.hpp:19-73)
  RegistrationIcpPointToPlane  <-> o3d_slam::RegistrationIcpPointToPlane (CloudRegistration.cpp:54-83)
  RegistrationIcpPointToPoint  <-> o3d_slam::RegistrationIcpPointToPoint (CloudRegistration.cpp:84-101)
  cloudRegistrationFactory     <-> o3d_slam::cloudRegistrationFactory (CloudRegistration.cpp:104-119)
  computeIndicesOfOverlappingPoints <-> o3d_slam::computeIndicesOfOverlappingPoints (helpers.cpp:320-345)
  buildConstraint              <-> o3d_slam::buildConstraint (constraint_builders.cpp:43-90)
  refineLoopClosure            <-> the refinement of a loop-closure candidate (PlaceRecognition.cpp:97-149)
  ComputeFPFHFeature           <-> open3d::pipelines::registration::ComputeFPFHFeature with KDTreeSearchParamHybrid
  CorrespondencesFromFeatures  <-> the feature-matching front of RegistrationRANSACBasedOnFeatureMatching
                                   (PlaceRecognition.cpp:81-84)
  computeSubmapFeatures        <-> o3d_slam::Submap::computeFeatures (Submap.cpp:255-275)
  RegistrationRANSACBasedOnCorrespondence / RegistrationRANSACBasedOnFeatureMatching
                               <-> the Open3D operators of the same names (PlaceRecognition.cpp:78-85)
  ransacLoopClosure            <-> the RANSAC step of a loop-closure candidate and its size check (PlaceRecognition.cpp:78-91)
  TransformInterpolationBuffer <-> o3d_slam::TransformInterpolationBuffer, interpolate and getTransform
                                   (TransformInterpolationBuffer.cpp, Transform.cpp:16-67); host arithmetic
  ConstantVelocityMotionCompensation <-> the class of the same name (MotionCompensation.cpp:30-139); the velocity estimate
                                   is host arithmetic, the undistortion runs on the device
  OptimizationProblem, GlobalOptimization, transformSubmaps <-> o3d_slam::OptimizationProblem (OptimizationProblem.cpp),
                                   Open3D's GlobalOptimization and SubmapCollection::transform (SubmapCollection.cpp:322-373)

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
    descriptor `normals` N x 3, `covariances` N x 6, and any other named descriptor in `descriptors` (name -> N x span
    fp32, e.g. `densities`, `observationDirections`); the filter chains see all of them as named descriptors."""
    features: np.ndarray
    normals: np.ndarray | None = None
    covariances: np.ndarray | None = None
    descriptors: dict = field(default_factory=dict)

    def getNbPoints(self) -> int:
        return 0 if self.features is None else int(np.asarray(self.features).shape[0])


def _translate(e: RegError):
    if e.status == 3:
        return ConvergenceError(str(e))
    if e.status == 7:
        return InvalidField(str(e))
    if e.status == 6:
        return InvalidParameter(str(e))
    if e.status == capi.OUT_OF_BOUNDS:   # BoundTransformationChecker (TransformationCheckersImpl.cpp:217-224)
        return ConvergenceError(str(e).split(": ", 1)[-1])
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
                if p.smooth_len > capi.SMOOTH_LEN_MAX:     # reg_create refuses it as well
                    raise InvalidParameter(f"smoothLength: at most {capi.SMOOTH_LEN_MAX} on the accelerated path")
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
            self._set_reference(referenceIn)
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
            self._set_reading(readingIn)
            T_out, res = self._reg.register(T)
        except RegError as e:
            self.last_result = getattr(self._reg, "last_result", None)   # filled on REG_OUT_OF_BOUNDS as well
            raise _translate(e) from None
        self.last_result = res
        self.maxNumIterationsReached = bool(res.max_iter_reached)
        return T_out

    def __call__(self, readingIn, referenceIn, T_refIn_readIn=None):
        return self.compute(readingIn, referenceIn, T_refIn_readIn, True)

    def _set_reference(self, referenceIn: DataPoints):
        self._reg.set_target(referenceIn.features, referenceIn.normals, referenceIn.covariances)

    def _set_reading(self, readingIn: DataPoints):
        self._reg.set_source(readingIn.features, readingIn.normals, readingIn.covariances)


class ErrorMinimizerView:
    """The getters of PointMatcher<T>::ErrorMinimizer a caller reads after ICP::compute (ErrorMinimizer.cpp:249-285,
    PointToPlane.cpp:780-930, PointToPlaneWithCov.cpp:165-169), for the last compute() of a PointMatcherICP."""

    def __init__(self, icp: "PointMatcherICP"):
        self._icp = icp

    def _stats(self):
        if self._icp._reg is None:
            raise RuntimeError("no registration has run")
        try:
            return self._icp._reg.get_minimizer_stats()
        except RegError as e:
            raise _translate(e) from None

    def getCovariance(self) -> np.ndarray:
        """6x6, order [x y z alpha beta gamma]; the zero matrix unless the minimizer is PointToPlaneWithCovErrorMinimizer
        (the base class, ErrorMinimizer.cpp:281-285)."""
        chain = self._icp.chain
        if chain is None or not chain.with_cov:
            return np.zeros((6, 6), np.float32)
        if self._icp._reg is None:
            raise RuntimeError("no registration has run")
        try:
            return self._icp._reg.get_covariance()[0]
        except RegError as e:
            raise _translate(e) from None

    def getOverlap(self) -> float:
        return float(self._stats().overlap)

    def getPointUsedRatio(self) -> float:
        return float(self._stats().point_used_ratio)

    def getWeightedPointUsedRatio(self) -> float:
        return float(self._stats().weighted_point_used_ratio)

    def getResidualError(self) -> float:
        return float(self._stats().residual_error)


class PointMatcherICP(ICP):
    """ICP with the libpointmatcher chain extension (include/o3dslam_reg.h, reg_set_pm_chain): loadFromYaml also takes
    KDTreeMatcher.knn up to 16, RobustOutlierFilter (OutlierFiltersImpl.h:230-244 names and defaults),
    MinDistOutlierFilter, MedianDistOutlierFilter, VarTrimmedDistOutlierFilter (OutlierFiltersImpl.h:96-160),
    PointToPointErrorMinimizer, PointToPlaneWithCovErrorMinimizer (sensorStdDev), BoundTransformationChecker
    (maxRotationNorm, maxTranslationNorm; its place relative to the Counter checker is kept) and degeneracyAwareness
    SolutionRemapping (threshold, use2019) or EqualityConstraints (all five keys; `localizability` holds its last
    analysis); everything else binds exactly as for ICP.  The robust filter's scale /
    iteration persist across compute() calls on the same object, as in the reference.  `errorMinimizer` holds the
    minimizer's getters (covariance, overlap, ratios, residual) of the last compute().

    PointToPlaneWithCovErrorMinimizer together with OptimizedEqualityConstraints: the reference runs the localizability
    detection only when the minimizer's name is exactly PointToPlaneErrorMinimizer (ICP.cpp:1114,1138) and the flags
    start as localizable (PointMatcher.h:638-639), so the constrained solve is the plain one; the parameters are
    checked and the analysis is switched off (params.use_xicp = 0)."""

    _ROBUST_DEFAULTS = {"robustFct": "cauchy", "tuning": 1.0, "scaleEstimator": "mad", "nbIterationForScale": 0,
                        "distanceType": "point2point", "approximation": math.inf}
    # filter -> ({parameter: default}, chain switch, {parameter: chain field})
    _DIST_FILTERS = {
        "MinDistOutlierFilter": ({"minDist": 1.0}, "use_min_dist_filter", {"minDist": "outlier_min_dist"}),
        "MedianDistOutlierFilter": ({"factor": 3.0}, "use_median_dist", {"factor": "median_factor"}),
        "VarTrimmedDistOutlierFilter": ({"minRatio": 0.05, "maxRatio": 0.99, "lambda": 2.35}, "use_var_trimmed",
                                        {"minRatio": "var_min_ratio", "maxRatio": "var_max_ratio", "lambda": "var_lambda"}),
    }

    # degeneracyAwareness EqualityConstraints (X-ICP, ternary): yaml key -> reg_ternary_xicp field (ICP.cpp:671-721)
    _TERNARY_KEYS = {"highInformationThreshold": "high_information", "enoughInformationThreshold": "enough_information",
                     "insufficientInformationThreshold": "insufficient_information",
                     "point2NormalMinimalAlignmentAngleThreshold": "min_alignment_angle_deg",
                     "point2NormalStrongAlignmentAngleThreshold": "strong_alignment_angle_deg"}

    def __init__(self):
        super().__init__()
        self.chain: capi.PmChainV3 | None = None
        self.ternary: capi.TernaryXicp | None = None
        self.referenceDataPointsFilters: list = []
        self.readingDataPointsFilters: list = []   # reg_filter_points specs and OctreeGridDataPointsFilter steps
        self._dev: dict = {}
        self._read_stages: list = []
        self._read_fields: dict = {}
        self.errorMinimizer = ErrorMinimizerView(self)

    def setDefault(self):
        super().setDefault()
        self.chain = None
        self.ternary = None
        self.referenceDataPointsFilters, self.readingDataPointsFilters = [], []

    def loadFromYaml(self, stream_or_text):
        """Also binds referenceDataPointsFilters (SamplingSurfaceNormal, SurfaceNormal, OctreeGrid) and
        readingDataPointsFilters (READING_FILTERS, DESCRIPTOR_FILTERS, SurfaceNormal, OctreeGrid) to the device filters
        (reg_sampling_surface_normal, reg_estimate_normals, reg_filter_points, reg_filter_cloud, reg_octree_grid)."""
        import yaml
        text = stream_or_text.read() if hasattr(stream_or_text, "read") else stream_or_text
        doc = yaml.safe_load(text) or {}
        ref_filters = [_reference_filter(f) for f in (doc.pop("referenceDataPointsFilters", None) or [])]
        read_filters = [_reading_filter(f) for f in (doc.pop("readingDataPointsFilters", None) or [])]
        chain = capi.default_pm_chain_v3()
        m = doc.get("matcher")
        if isinstance(m, dict) and isinstance(m.get("KDTreeMatcher"), dict) and "knn" in m["KDTreeMatcher"]:
            chain.knn = int(m["KDTreeMatcher"]["knn"])
            m["KDTreeMatcher"] = dict(m["KDTreeMatcher"], knn=1)
        kept = []
        for f in doc.get("outlierFilters") or []:
            (fname, fargs), = (f.items() if isinstance(f, dict) else [(f, {})])
            if fname in self._DIST_FILTERS:
                self._bind_dist_filter(chain, fname, fargs or {})
                continue
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
        (emname, emargs), = (em.items() if isinstance(em, dict) else [(em, {})])
        emargs = emargs or {}
        if emname == "PointToPointErrorMinimizer":
            chain.minimizer = capi.PM_POINT_TO_POINT
            doc["errorMinimizer"] = "PointToPlaneErrorMinimizer"
        elif emname == "PointToPointWithCovErrorMinimizer":
            raise NotImplementedError("PointToPointWithCovErrorMinimizer: its estimate sets normal = (1,1,1) "
                                      "(PointToPointWithCov.cpp:77), so H is singular by construction and the result is "
                                      "the output of an LU on a rank-deficient matrix")
        elif emname == "PointToPlaneWithCovErrorMinimizer":
            unknown = set(emargs) - {"sensorStdDev", "force2D", "force4DOF"}
            if unknown:
                raise InvalidParameter(f"PointToPlaneWithCovErrorMinimizer: unknown parameter(s) {sorted(unknown)}")
            try:
                chain.sensor_std_dev = float(emargs.get("sensorStdDev", 0.01))
                forced = float(emargs.get("force2D", 0)) != 0 or float(emargs.get("force4DOF", 0)) != 0
            except (TypeError, ValueError):
                raise InvalidParameter("PointToPlaneWithCovErrorMinimizer: parameters must be numbers") from None
            if forced:
                raise NotImplementedError("PointToPlaneWithCovErrorMinimizer: force2D / force4DOF are outside the "
                                          "accelerated path")
            chain.with_cov = 1
            doc["errorMinimizer"] = "PointToPlaneErrorMinimizer"
        checkers, counter_seen = [], False
        for c in doc.get("transformationCheckers") or []:
            (cname, cargs), = (c.items() if isinstance(c, dict) else [(c, {})])
            if cname == "CounterTransformationChecker":
                counter_seen = True
            if cname != "BoundTransformationChecker":
                checkers.append(c)
                continue
            if chain.use_bound:
                raise NotImplementedError("more than one BoundTransformationChecker")
            cargs = cargs or {}
            unknown = set(cargs) - {"maxRotationNorm", "maxTranslationNorm"}
            if unknown:
                raise InvalidParameter(f"BoundTransformationChecker: unknown parameter(s) {sorted(unknown)}")
            try:
                chain.max_rotation_norm = float(cargs.get("maxRotationNorm", 1.0))
                chain.max_translation_norm = float(cargs.get("maxTranslationNorm", 1.0))
            except (TypeError, ValueError):
                raise InvalidParameter("BoundTransformationChecker: parameters must be numbers") from None
            if not (chain.max_rotation_norm >= 0 and chain.max_translation_norm >= 0):
                raise InvalidParameter("BoundTransformationChecker: maxRotationNorm / maxTranslationNorm must be >= 0")
            chain.use_bound = 1
            chain.bound_after_counter = 1 if counter_seen else 0
        if "transformationCheckers" in doc:
            doc["transformationCheckers"] = checkers
        da = doc.get("degeneracyAwareness")
        if da == "SolutionRemapping":
            da = {"SolutionRemapping": None}
        if isinstance(da, dict) and "SolutionRemapping" in da:
            if len(da) != 1:
                raise InvalidParameter("degeneracyAwareness: one method at a time")
            dargs = da["SolutionRemapping"] or {}
            if "threshold" not in dargs or "use2019" not in dargs:     # ICP.cpp:603-627
                raise InvalidParameter("SolutionRemapping needs threshold, use2019")
            unknown = set(dargs) - {"threshold", "use2019"}
            if unknown:
                raise InvalidParameter(f"SolutionRemapping: unknown parameter(s) {sorted(unknown)}")
            try:
                chain.sr_threshold = float(dargs["threshold"])
                chain.sr_use2019 = 1 if float(dargs["use2019"]) == 1.0 else 0
            except (TypeError, ValueError):
                raise InvalidParameter("SolutionRemapping: parameters must be numbers") from None
            chain.degeneracy_method = capi.DEGENERACY_SOLUTION_REMAPPING
            doc.pop("degeneracyAwareness")
        ternary = None
        if isinstance(da, dict) and "EqualityConstraints" in da and isinstance(da["EqualityConstraints"], dict):
            if len(da) != 1:
                raise InvalidParameter("degeneracyAwareness: one method at a time")
            dargs = da["EqualityConstraints"]
            unknown = set(dargs) - set(self._TERNARY_KEYS)
            if unknown:
                raise InvalidParameter(f"EqualityConstraints: unknown parameter(s) {sorted(unknown)}")
            # a block without all five keys is one the reference itself rejects (ICP.cpp:674-720 returns false): it stays
            # with the base class, which refuses the method
            if all(k in dargs for k in self._TERNARY_KEYS):
                ternary = capi.default_ternary_xicp(True)
                try:
                    for key, field in self._TERNARY_KEYS.items():
                        if isinstance(dargs[key], (bool, str)) or dargs[key] is None:
                            raise TypeError(key)
                        setattr(ternary, field, float(dargs[key]))
                except (TypeError, ValueError):
                    raise InvalidParameter("EqualityConstraints: parameters must be numbers") from None
                doc.pop("degeneracyAwareness")
        super().loadFromYaml(yaml.safe_dump(doc))
        if chain.with_cov and self.params.use_xicp:
            self.params.use_xicp = 0   # the reference skips the detection for this minimizer (class docstring)
        if chain.with_cov:
            ternary = None             # ... and likewise for EqualityConstraints
        if ternary is not None:
            st = capi.check_ternary_xicp(self.params, chain, ternary)
            if st == 9:
                raise NotImplementedError("EqualityConstraints runs with point-to-plane, knn 1 and the 0/1-weight outlier "
                                          "filters only (no RobustOutlierFilter, no point-to-point)")
            if st != 0:
                raise InvalidParameter("EqualityConstraints: thresholds must be finite and ordered insufficient <= enough "
                                       "<= high, angles must lie in (0, 90]")
        st = capi.check_pm_chain(self.params, chain)
        if st == 9:
            raise NotImplementedError("this chain is outside the accelerated path (std scale estimator; X-ICP with "
                                      "k-NN / robust weights / point-to-point / MinDist / MedianDist / VarTrimmedDist / "
                                      "BoundTransformationChecker; SolutionRemapping or a covariance with point-to-point)")
        if st != 0:
            raise InvalidParameter("invalid chain (knn must lie in 1..16; a filter parameter out of range; "
                                   "VarTrimmedDistOutlierFilter: minRatio should be smaller than maxRatio)")
        self.chain = chain
        self.ternary = ternary
        self.referenceDataPointsFilters, self.readingDataPointsFilters = ref_filters, read_filters

    @classmethod
    def _bind_dist_filter(cls, chain, fname, fargs):
        """MinDist / MedianDist / VarTrimmedDist -> the chain's fields; the ranges are checked by reg_check_pm_chain."""
        defaults, switch, fields = cls._DIST_FILTERS[fname]
        if getattr(chain, switch):
            raise NotImplementedError(f"more than one {fname}")
        unknown = set(fargs) - set(defaults)
        if unknown:
            raise InvalidParameter(f"{fname}: unknown parameter(s) {sorted(unknown)}")
        setattr(chain, switch, 1)
        for name, value in dict(defaults, **fargs).items():
            try:
                setattr(chain, fields[name], float(value))
            except (TypeError, ValueError):
                raise InvalidParameter(f"{fname}: {name} must be a number") from None

    def _buf(self, key, nbytes):
        b = self._dev.get(key)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self._dev[key] = capi.DeviceArray(nbytes)
        return b

    def _set_reference(self, referenceIn: DataPoints):
        """ICP::initReference: the reference filters run on the device and their output goes to reg_set_target as
        device pointers (ICP.cpp:864-866: before the centroid)."""
        if not self.referenceDataPointsFilters:
            return super()._set_reference(referenceIn)
        x = np.ascontiguousarray(referenceIn.features, np.float32)
        n, stride = x.shape[0], x.shape[1]
        src = self._buf("ref_in", x.nbytes)
        src.upload(x)
        cur, cur_stride, nrm = src.value, stride, None
        if referenceIn.normals is not None and any(isinstance(f, OctreeGridDataPointsFilter)
                                                   for f in self.referenceDataPointsFilters):
            nb = self._buf("ref_nrm_in", n * 12)   # an octree step carries the descriptors it is given
            nb.upload(np.ascontiguousarray(referenceIn.normals, np.float32))
            nrm = nb.value
        for i, f in enumerate(self.referenceDataPointsFilters):
            if isinstance(f, OctreeGridDataPointsFilter):
                ox = self._buf(f"ref_xyz{i}", n * 12)
                on = self._buf(f"ref_nrm{i}", n * 12) if nrm is not None else None
                n = self._reg.octree_grid_device(cur, cur_stride, n, f.params(), ox.value, nrm, None,
                                                 on.value if on is not None else None)
                cur, cur_stride, nrm = ox.value, 3, (on.value if on is not None else None)
            elif isinstance(f, SamplingSurfaceNormalDataPointsFilter):
                ox, on = self._buf(f"ref_xyz{i}", n * 12), self._buf(f"ref_nrm{i}", n * 12)
                n, _ = self._reg.sampling_surface_normal_device(cur, cur_stride, n, f.params(), ox.value,
                                                                on.value if f.keepNormals else None)
                cur, cur_stride, nrm = ox.value, 3, (on.value if f.keepNormals else None)
            else:   # SurfaceNormalDataPointsFilter: normals of the current points, xyz unchanged
                on = self._buf(f"ref_nrm{i}", n * 12)
                self._reg.estimate_normals_device(cur, cur_stride, n, on.value, k=f.knn, max_dist=f.maxDist,
                                                  viewpoint=f.viewpoint)
                if f.keepNormals:
                    nrm = on.value
        self._reg.set_target_device(cur, cur_stride, n, nrm, 3, None)
        self.referenceFilteredCount = n

    def _set_reading(self, readingIn: DataPoints):
        """ICP::computeWithTransformedReference (ICP.cpp:950-955): the reading filters run on the device before the
        reading's centroid; reg_set_source reads their output in place.  Correspondence ids index the filtered cloud."""
        self._read_fields = {}
        if not self.readingDataPointsFilters:
            self._read_stages = []
            return super()._set_reading(readingIn)
        if readingIn.descriptors or _needs_fields(self.readingDataPointsFilters):
            return self._set_reading_fields(readingIn)
        x = np.ascontiguousarray(readingIn.features, np.float32)
        n, stride = x.shape[0], x.shape[1]
        src = self._buf("read_in", x.nbytes)
        src.upload(x)
        nin = cin = None
        if readingIn.normals is not None:
            nin = self._buf("read_nrm_in", n * 12)
            nin.upload(np.ascontiguousarray(readingIn.normals, np.float32))
        if readingIn.covariances is not None:
            cin = self._buf("read_cov_in", n * 24)
            cin.upload(np.ascontiguousarray(readingIn.covariances, np.float32))
        cur, cur_stride = src.value, stride
        cur_nrm, cur_cov = (nin.value if nin else None), (cin.value if cin else None)
        self._read_stages = []
        # runs of point filters go to reg_filter_points in one call; every octree step is a reg_octree_grid call
        stages, run = [], []
        for f in self.readingDataPointsFilters:
            if isinstance(f, OctreeGridDataPointsFilter):
                if run:
                    stages.append(run)
                stages.append(f)
                run = []
            else:
                run.append(f)
        if run or not stages:
            stages.append(run)
        for k, st in enumerate(stages):
            sfx = "" if k == 0 else str(k)
            ox, oi = self._buf("read_xyz" + sfx, n * 12), self._buf("read_idx" + sfx, n * 4)
            on = self._buf("read_nrm" + sfx, n * 12) if cur_nrm is not None else None
            oc = self._buf("read_cov" + sfx, n * 24) if cur_cov is not None else None
            if isinstance(st, OctreeGridDataPointsFilter):
                m = self._reg.octree_grid_device(cur, cur_stride, n, st.params(), ox.value, cur_nrm, cur_cov,
                                                 on.value if on else None, oc.value if oc else None, oi.value)
            else:
                m = self._reg.filter_points_device(cur, cur_stride, n, st, ox.value, cur_nrm, cur_cov,
                                                   on.value if on else None, oc.value if oc else None, oi.value)
            if m == 0:
                raise RuntimeError("The reading point cloud is empty.")   # ICP.cpp:958-960
            self._read_stages.append(("read_idx" + sfx, m))
            cur, cur_stride, n = ox.value, 3, m
            cur_nrm, cur_cov = (on.value if on else None), (oc.value if oc else None)
        self._reg.set_source_device(cur, 3, n, cur_nrm, 3, cur_cov)
        self.readingFilteredCount = n

    def _set_reading_fields(self, readingIn: DataPoints):
        """The reading chain with named descriptors (run_filter_chain): every field stays on the device; the final
        `normals` / `covariances` fields go to reg_set_source."""
        _check_fields(self.readingDataPointsFilters, _cloud_fields(readingIn))
        cur, stride, n, fields, stages = run_filter_chain(self._reg, self._buf, "read", self.readingDataPointsFilters,
                                                          readingIn)
        if n == 0:
            raise RuntimeError("The reading point cloud is empty.")   # ICP.cpp:958-960
        self._read_stages, self._read_fields = stages, dict(fields, _n=n)
        nrm, cov = fields.get("normals"), fields.get("covariances")
        self._reg.set_source_device(cur, stride, n, nrm[0] if nrm else None, 3, cov[0] if cov else None)
        self.readingFilteredCount = n

    def readingFilteredIndices(self) -> np.ndarray:
        """Source index (into the last compute()'s reading) of every filtered reading point, composed through every
        step of the chain."""
        idx = None
        for key, m in self._read_stages:
            step = self._dev[key].download(m, np.int32)
            idx = step if idx is None else idx[step]
        if idx is None and self._read_fields:
            idx = np.arange(self._read_fields["_n"], dtype=np.int32)   # a chain without a compaction
        return idx

    def readingFilteredDescriptor(self, name: str) -> np.ndarray:
        """The descriptor `name` (n x span) of the last compute()'s filtered reading, downloaded from the device."""
        if name == "_n" or name not in self._read_fields:
            raise InvalidField(f"Cannot find descriptor {name}")
        ptr, span = self._read_fields[name]
        return capi.download(ptr, (self._read_fields["_n"], span))

    def _ensure(self):
        fresh = self._reg is None
        super()._ensure()
        if fresh and self.chain is not None:
            try:
                self._reg.set_pm_chain(self.chain)
            except RegError as e:
                raise _translate(e) from None
        if fresh and self.ternary is not None:
            try:
                self._reg.set_ternary_xicp(self.ternary)
            except RegError as e:
                raise _translate(e) from None

    @property
    def localizability(self) -> "capi.TernaryXicpResult":
        """The EqualityConstraints analysis of the last compute()'s last iteration (reg_get_ternary_xicp)."""
        if self._reg is None:
            raise RuntimeError("no registration has run")
        try:
            return self._reg.get_ternary_xicp()
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


class SamplingSurfaceNormalDataPointsFilter:
    """SamplingSurfaceNormalDataPointsFilter (DataPointsFilters/SamplingSurfaceNormal.{h,cpp}) on the device
    (reg_sampling_surface_normal), parameters by the reference's names and defaults.  samplingMethod 0 with ratio < 1
    draws from std::rand and is refused (NotImplementedError); averageExistingDescriptors has no effect (no descriptors
    are carried).  `filter` returns the sampled DataPoints; densities / eigen outputs stay on the filter."""

    PARAMS = {"ratio": 0.5, "knn": 7, "samplingMethod": 0, "maxBoxDim": math.inf, "averageExistingDescriptors": 1,
              "keepNormals": 1, "keepDensities": 0, "keepEigenValues": 0, "keepEigenVectors": 0}

    def __init__(self, **kw):
        unknown = set(kw) - set(self.PARAMS)
        if unknown:
            raise InvalidParameter(f"SamplingSurfaceNormalDataPointsFilter: unknown parameter(s) {sorted(unknown)}")
        a = dict(self.PARAMS, **kw)
        self.ratio, self.knn, self.samplingMethod = float(a["ratio"]), int(a["knn"]), int(a["samplingMethod"])
        self.maxBoxDim, self.averageExistingDescriptors = float(a["maxBoxDim"]), bool(int(a["averageExistingDescriptors"]))
        self.keepNormals, self.keepDensities = bool(int(a["keepNormals"])), bool(int(a["keepDensities"]))
        self.keepEigenValues, self.keepEigenVectors = bool(int(a["keepEigenValues"])), bool(int(a["keepEigenVectors"]))
        if self.knn < 3:
            raise InvalidParameter("knn: minimum 3 (SamplingSurfaceNormal.h)")
        if self.samplingMethod not in (0, 1):
            raise InvalidParameter("samplingMethod: 0 or 1")
        if self.knn > 64:
            raise NotImplementedError("SamplingSurfaceNormalDataPointsFilter: knn above 64 is not supported on the device")
        if self.samplingMethod == 0 and self.ratio < 1:
            raise NotImplementedError("SamplingSurfaceNormalDataPointsFilter: samplingMethod 0 with ratio < 1 draws from "
                                      "std::rand, which cannot be reproduced")
        self.densities = self.eigValues = self.eigVectors = None
        self._reg = None

    def params(self) -> capi.SsnParams:
        p = capi.default_ssn_params()
        p.knn, p.sampling_method, p.ratio, p.max_box_dim = self.knn, self.samplingMethod, self.ratio, self.maxBoxDim
        p.average_existing_descriptors = int(self.averageExistingDescriptors)
        p.keep_normals, p.keep_densities = int(self.keepNormals), int(self.keepDensities)
        p.keep_eigen_values, p.keep_eigen_vectors = int(self.keepEigenValues), int(self.keepEigenVectors)
        return p

    def filter(self, cloud: DataPoints) -> DataPoints:
        if self._reg is None:
            self._reg = capi.Registration(capi.default_params())
        try:
            out = self._reg.sampling_surface_normal(cloud.features, self.params())
        except RegError as e:
            raise _translate(e) from None
        self.densities, self.eigValues, self.eigVectors = out.get("densities"), out.get("eigvals"), out.get("eigvecs")
        return DataPoints(out["xyz"], out.get("normals"), None)


class OctreeGridDataPointsFilter:
    """OctreeGridDataPointsFilter (DataPointsFilters/OctreeGrid.{h,cpp}, utils/octree) on the device (reg_octree_grid),
    parameters by the reference's names and defaults.  Row k of the output is the sample of the k-th non-empty leaf in
    depth-first order (the documented deviation from the samplers' swapCols bookkeeping); samplingMethod 1
    replays glibc's rand() after srand(1), as RandomPtsSampler does on every call.  Normals and covariances are carried
    (CENTROID averages them).  After `filter`, srcIdx / leafId / leafDepth hold the last call's indices."""

    PARAMS = {"buildParallel": 1, "maxPointByNode": 1, "maxSizeByNode": 0.0, "samplingMethod": 0, "centerAtOrigin": 1}

    def __init__(self, **kw):
        unknown = set(kw) - set(self.PARAMS)
        if unknown:
            raise InvalidParameter(f"OctreeGridDataPointsFilter: unknown parameter(s) {sorted(unknown)}")
        a = dict(self.PARAMS, **kw)
        try:
            self.maxPointByNode, self.maxSizeByNode = int(a["maxPointByNode"]), float(a["maxSizeByNode"])
            self.samplingMethod = int(a["samplingMethod"])
            flags = {k: int(a[k]) for k in ("buildParallel", "centerAtOrigin")}
        except (TypeError, ValueError):
            raise InvalidParameter("OctreeGridDataPointsFilter: parameters must be numbers") from None
        if not 1 <= self.maxPointByNode <= 4294967295:
            raise InvalidParameter("maxPointByNode: must lie in 1..4294967295 (OctreeGrid.h)")
        if not self.maxSizeByNode >= 0:
            raise InvalidParameter("maxSizeByNode: must be >= 0 (OctreeGrid.h)")
        if self.samplingMethod not in (0, 1, 2, 3):
            raise InvalidParameter("samplingMethod: 0 (first), 1 (random), 2 (centroid) or 3 (medoid)")
        if any(v not in (0, 1) for v in flags.values()):
            raise InvalidParameter("buildParallel / centerAtOrigin: 0 or 1")
        self.buildParallel, self.centerAtOrigin = bool(flags["buildParallel"]), bool(flags["centerAtOrigin"])
        self.srcIdx = self.leafId = self.leafDepth = None
        self._reg = None

    def params(self) -> capi.OctreeParams:
        return capi.default_octree_params(max_point_by_node=self.maxPointByNode, max_size_by_node=self.maxSizeByNode,
                                          sampling_method=self.samplingMethod, center_at_origin=int(self.centerAtOrigin),
                                          build_parallel=int(self.buildParallel))

    def filter(self, cloud: DataPoints) -> DataPoints:
        if self._reg is None:
            self._reg = capi.Registration(capi.default_params())
        try:
            out = self._reg.octree_grid(cloud.features, self.params(), cloud.normals, cloud.covariances)
        except RegError as e:
            raise _translate(e) from None
        self.srcIdx, self.leafId, self.leafDepth = out["src_idx"], out["leaf_id"], out["leaf_depth"]
        return DataPoints(out["xyz"], out.get("normals"), out.get("covs"))


class VoxelGridDataPointsFilter:
    """VoxelGridDataPointsFilter (DataPointsFilters/VoxelGrid.{h,cpp}) on the device (reg_voxel_grid), parameters by the
    reference's names and defaults.  useCentroid 0 is refused: that branch of this fork writes the cell centre into
    feature rows 1..3 -- y, z and the homogeneous pad (VoxelGrid.cpp:289-304) -- and the reference's own test never runs
    it (DataFilters.cpp:638-672).  Every descriptor is carried (averaged with averageExistingDescriptors, else the
    voxel's first member's).  A stage of parse_filters / filter_cloud chains and of an assigned
    `readingDataPointsFilters`; loadFromYaml keeps refusing the name (see _reading_filter)."""

    PARAMS = {"vSizeX": 1.0, "vSizeY": 1.0, "vSizeZ": 1.0, "useCentroid": 1, "averageExistingDescriptors": 1}

    def __init__(self, **kw):
        unknown = set(kw) - set(self.PARAMS)
        if unknown:
            raise InvalidParameter(f"VoxelGridDataPointsFilter: unknown parameter(s) {sorted(unknown)}")
        a = dict(self.PARAMS, **kw)
        try:
            self.vSize = tuple(float(a[k]) for k in ("vSizeX", "vSizeY", "vSizeZ"))
            flags = {k: int(a[k]) for k in ("useCentroid", "averageExistingDescriptors")}
        except (TypeError, ValueError):
            raise InvalidParameter("VoxelGridDataPointsFilter: parameters must be numbers") from None
        if not all(0.001 <= v < math.inf for v in self.vSize):
            raise InvalidParameter("vSizeX / vSizeY / vSizeZ: must lie in [0.001, inf) (VoxelGrid.h)")
        if any(v not in (0, 1) for v in flags.values()):
            raise InvalidParameter("useCentroid / averageExistingDescriptors: 0 or 1")
        if not flags["useCentroid"]:
            raise NotImplementedError("VoxelGridDataPointsFilter: useCentroid 0 writes the cell centre into feature rows "
                                      "1..3 in the reference (VoxelGrid.cpp:289-304); only useCentroid 1 is built")
        self.useCentroid, self.averageExistingDescriptors = True, bool(flags["averageExistingDescriptors"])
        self.srcIdx = None
        self._reg = None

    def params(self) -> capi.VoxelGridParams:
        return capi.default_voxel_grid_params(self.vSize, 1, int(self.averageExistingDescriptors))

    def filter(self, cloud: DataPoints) -> DataPoints:
        out, self.srcIdx = filter_cloud([self], cloud, return_indices=True)
        return out


# readingDataPointsFilters bound to reg_filter_points: name -> {parameter: default} (each filter's .h)
READING_FILTERS = {
    "IdentityDataPointsFilter": {},
    "MaxDistDataPointsFilter": {"dim": -1, "maxDist": 1.0},
    "MinDistDataPointsFilter": {"dim": -1, "minDist": 1.0},
    "BoundingBoxDataPointsFilter": {"xMin": -1.0, "xMax": 1.0, "yMin": -1.0, "yMax": 1.0, "zMin": -1.0, "zMax": 1.0,
                                    "removeInside": 1},
    "DistanceLimitDataPointsFilter": {"dim": -1, "dist": 1.0, "removeInside": 1},
    "RemoveNaNDataPointsFilter": {},
    "MaxQuantileOnAxisDataPointsFilter": {"dim": 0, "ratio": 0.5},
    # phase: the reference draws rand() % step on every compute; here it is explicit (default 0)
    "FixStepSamplingDataPointsFilter": {"startStep": 10, "endStep": 10, "stepMult": 1.0, "phase": 0},
}
# Descriptor filters bound to reg_filter_cloud: name -> {parameter: default} (each filter's .h).  MaxDensity's seed: the
# reference continues the process-wide std::rand stream; here every call replays rand() after srand(seed).
DESCRIPTOR_FILTERS = {
    "ObservationDirectionDataPointsFilter": {"x": 0.0, "y": 0.0, "z": 0.0},
    "OrientNormalsDataPointsFilter": {"towardCenter": 1},
    "ShadowDataPointsFilter": {"eps": 0.1},
    "SimpleSensorNoiseDataPointsFilter": {"sensorType": 0, "gain": 1.0},
    "IncidenceAngleDataPointsFilter": {},
    "CutAtDescriptorThresholdDataPointsFilter": {"descName": "none", "useLargerThan": 1, "threshold": 0.0},
    "MaxDensityDataPointsFilter": {"maxDensity": 10.0, "seed": 1},
}
_REFUSED_FILTERS = {
    "RandomSamplingDataPointsFilter": "draws from std::rand, which cannot be reproduced",
    "MaxPointCountDataPointsFilter": "subsamples with std::rand above maxCount",
}


def _split(f):
    (name, args), = (f.items() if isinstance(f, dict) else [(f, {})])
    return name, dict(args or {})


def _descriptor_filter(name, args):
    unknown = set(args) - set(DESCRIPTOR_FILTERS[name])
    if unknown:
        raise InvalidParameter(f"{name}: unknown parameter(s) {sorted(unknown)}")
    spec = dict(DESCRIPTOR_FILTERS[name], **args)
    spec["type"] = name[:-len("DataPointsFilter")]
    try:
        for k, v in spec.items():
            if k not in ("type", "descName"):
                spec[k] = float(v) if isinstance(DESCRIPTOR_FILTERS[name][k], float) else int(v)
    except (TypeError, ValueError):
        raise InvalidParameter(f"{name}: parameters must be numbers") from None
    t = spec["type"]
    if t == "SimpleSensorNoise" and not 0 <= spec["sensorType"] <= 4:
        raise InvalidParameter(f"SimpleSensorNoiseDataPointsFilter: Error, sensorType id {spec['sensorType']} does not exist.")
    if t == "SimpleSensorNoise" and not spec["gain"] >= 1:
        raise InvalidParameter("SimpleSensorNoiseDataPointsFilter: gain must be >= 1")
    if t == "Shadow" and not 0.0 <= spec["eps"] <= 3.1416:
        raise InvalidParameter("ShadowDataPointsFilter: eps must lie in [0, 3.1416]")
    if t == "MaxDensity" and not spec["maxDensity"] >= 0.0000001:
        raise InvalidParameter("MaxDensityDataPointsFilter: maxDensity must be >= 0.0000001")
    if t == "MaxDensity" and not 1 <= spec["seed"] <= 0x7fffffff:
        raise InvalidParameter("MaxDensityDataPointsFilter: seed must lie in 1..2147483647")
    if t in ("OrientNormals", "CutAtDescriptorThreshold"):
        key = "towardCenter" if t == "OrientNormals" else "useLargerThan"
        if spec[key] not in (0, 1):
            raise InvalidParameter(f"{name}: {key} must be 0 or 1")
    return spec


def _surface_normal_filter(args, where):
    known = {"knn", "maxDist", "epsilon", "keepNormals", "keepDensities", "keepEigenValues", "keepEigenVectors",
             "keepMatchedIds", "keepMeanDist", "sortEigen", "smoothNormals"}
    unknown = set(args) - known
    if unknown:
        raise InvalidParameter(f"SurfaceNormalDataPointsFilter: unknown parameter(s) {sorted(unknown)}")
    if int(args.pop("smoothNormals", 0)):
        raise NotImplementedError(f"SurfaceNormalDataPointsFilter: smoothNormals in a {where} chain")
    args.pop("sortEigen", None)
    return SurfaceNormalDataPointsFilter(**{k: (bool(int(v)) if k.startswith("keep") else v) for k, v in args.items()})


def _reading_filter(f):
    """One entry of a yaml readingDataPointsFilters list.  VoxelGridDataPointsFilter is not bound here: a default
    VoxelGrid in a loaded reading chain is pinned to NotImplementedError (tests/test_data_filters_host.py,
    test_refused_chains_still_raise); parse_filters / filter_cloud take it (_chain_filter)."""
    name, args = _split(f)
    if name == "OctreeGridDataPointsFilter":
        return OctreeGridDataPointsFilter(**args)
    if name == "SurfaceNormalDataPointsFilter":
        return _surface_normal_filter(args, "reading")
    if name in DESCRIPTOR_FILTERS:
        return _descriptor_filter(name, args)
    if name in _REFUSED_FILTERS:
        raise NotImplementedError(f"{name}: {_REFUSED_FILTERS[name]}")
    if name not in READING_FILTERS:
        raise NotImplementedError(f"reading filter {name} is outside the accelerated path")
    unknown = set(args) - set(READING_FILTERS[name])
    if unknown:
        raise InvalidParameter(f"{name}: unknown parameter(s) {sorted(unknown)}")
    spec = dict(READING_FILTERS[name], **args)
    spec["type"] = name[:-len("DataPointsFilter")]
    if spec["type"] == "MaxQuantileOnAxis" and not (0 < float(spec["ratio"]) < 1):
        raise InvalidParameter("MaxQuantileOnAxisDataPointsFilter: ratio must lie in (0, 1)")
    if spec["type"] == "FixStepSampling" and int(spec["startStep"]) < 1:
        raise InvalidParameter("FixStepSamplingDataPointsFilter: startStep >= 1")
    return spec


def _reference_filter(f):
    name, args = _split(f)
    if name == "SamplingSurfaceNormalDataPointsFilter":
        return SamplingSurfaceNormalDataPointsFilter(**args)
    if name == "OctreeGridDataPointsFilter":
        return OctreeGridDataPointsFilter(**args)
    if name == "SurfaceNormalDataPointsFilter":
        return _surface_normal_filter(args, "reference")
    if name in _REFUSED_FILTERS:
        raise NotImplementedError(f"{name}: {_REFUSED_FILTERS[name]}")
    raise NotImplementedError(f"reference filter {name} is outside the accelerated path")


# ---- filter chains over named descriptors ----------------------------------------------------------------------------
# descriptors SurfaceNormalDataPointsFilter deposits in a chain: (switch, reference name, span, reg_estimate_normals output)
_SURFACE_NORMAL_FIELDS = (("keepNormals", "normals", 3, "normals_ptr"), ("keepDensities", "densities", 1, "densities_ptr"),
                          ("keepEigenValues", "eigValues", 3, "eigvals_ptr"),
                          ("keepEigenVectors", "eigVectors", 9, "eigvecs_ptr"), ("keepMeanDist", "meanDists", 1, "mean_dists_ptr"))


def _needs_fields(filters) -> bool:
    """True when the chain creates or reads a named descriptor or holds a VoxelGrid stage (it then runs through
    run_filter_chain)."""
    return any(isinstance(f, (SurfaceNormalDataPointsFilter, VoxelGridDataPointsFilter)) or
               (isinstance(f, dict) and f["type"] in capi.CLOUD_FILTERS)
               for f in filters)


def _cloud_fields(cloud: DataPoints) -> dict:
    """name -> span of the descriptors a cloud carries."""
    out = {}
    if cloud.normals is not None:
        out["normals"] = 3
    if cloud.covariances is not None:
        out["covariances"] = 6
    for name, a in (cloud.descriptors or {}).items():
        a = np.asarray(a)
        out[name] = 1 if a.ndim == 1 else int(a.shape[1])
    return out


def _check_fields(filters, have: dict) -> dict:
    """Walks the chain over the descriptor names: InvalidField where a filter reads a descriptor that does not exist at
    its place (as the reference throws), NotImplementedError where an octree step would have to carry other fields than
    normals / covariances.  Returns the names (-> span) after the chain."""
    have = dict(have)
    for f in filters:
        if isinstance(f, SurfaceNormalDataPointsFilter):
            for switch, name, span, _ in _SURFACE_NORMAL_FIELDS:
                if getattr(f, switch):
                    have[name] = span
        elif isinstance(f, OctreeGridDataPointsFilter):
            extra = sorted(set(have) - {"normals", "covariances"})
            if extra:
                raise NotImplementedError(f"OctreeGridDataPointsFilter: cannot carry the descriptors {extra}")
        elif isinstance(f, dict) and f["type"] in capi.CLOUD_FILTERS:
            _, a, b, made = capi.CLOUD_FILTERS[f["type"]]
            for need in (a, b):
                need = f.get("descName", "none") if need == "@descName" else need
                if need and need not in have:
                    raise InvalidField(f"{f['type']}DataPointsFilter: Error, cannot find {need} in descriptors.")
            if made:
                have[made[0]] = made[1]
    return have


def run_filter_chain(reg, buf, tag, filters, cloud: DataPoints):
    """Runs a parsed chain on the device.  `buf(key, nbytes)` hands out device buffers that stay valid until the next run.
    Stages: runs of point / descriptor filters are one reg_filter_cloud call each, SurfaceNormal is reg_estimate_normals
    (it adds fields, drops no point), OctreeGrid is reg_octree_grid.  Returns (xyz pointer, stride, n,
    {name: (pointer, span)}, [(key of the stage's source-index buffer, its length)])."""
    x = np.ascontiguousarray(cloud.features, np.float32)
    n, stride = x.shape[0], x.shape[1]
    src = buf(tag + "_in", x.nbytes)
    src.upload(x)
    cur = src.value
    fields = {}
    given = dict(cloud.descriptors or {})
    if cloud.normals is not None:
        given["normals"] = cloud.normals
    if cloud.covariances is not None:
        given["covariances"] = cloud.covariances
    for name, a in given.items():
        a = np.ascontiguousarray(a, np.float32).reshape(n, -1)
        b = buf(f"{tag}_in_{name}", a.nbytes)
        b.upload(a)
        fields[name] = (b.value, a.shape[1])
    stages, run = [], []
    for f in filters:
        if isinstance(f, dict):
            run.append(f)
        else:
            if run:
                stages.append(run)
            stages.append(f)
            run = []
    if run:
        stages.append(run)
    idx_stages = []
    for k, st in enumerate(stages):
        if n == 0:
            break
        if isinstance(st, SurfaceNormalDataPointsFilter):
            outs = {}
            for switch, name, span, arg in _SURFACE_NORMAL_FIELDS:
                if getattr(st, switch) or name == "normals":
                    outs[name] = (buf(f"{tag}_{k}_{name}", n * span * 4).value, span, arg)
            kw = {arg: ptr for name, (ptr, _, arg) in outs.items() if name != "normals"}
            reg.estimate_normals_device(cur, stride, n, outs["normals"][0], k=st.knn, max_dist=st.maxDist,
                                        viewpoint=st.viewpoint, **kw)
            for name, (ptr, span, _) in outs.items():
                if name != "normals" or st.keepNormals:
                    fields[name] = (ptr, span)
            continue
        ox, oi = buf(f"{tag}_{k}_xyz", n * 12), buf(f"{tag}_{k}_idx", n * 4)
        if isinstance(st, VoxelGridDataPointsFilter):
            flist = [(name, ptr, buf(f"{tag}_{k}_{name}", n * span * 4).value, span) for name, (ptr, span) in fields.items()]
            m = reg.voxel_grid_device(cur, stride, n, st.params(), flist, ox.value, oi.value)
            fields = {name: (out, span) for name, _, out, span in flist}
        elif isinstance(st, OctreeGridDataPointsFilter):
            nrm, cov = fields.get("normals"), fields.get("covariances")
            on = buf(f"{tag}_{k}_normals", n * 12) if nrm else None
            oc = buf(f"{tag}_{k}_covariances", n * 24) if cov else None
            m = reg.octree_grid_device(cur, stride, n, st.params(), ox.value, nrm[0] if nrm else None,
                                       cov[0] if cov else None, on.value if on else None, oc.value if oc else None, oi.value)
            fields = {name: (b.value, span) for name, b, span in (("normals", on, 3), ("covariances", oc, 6)) if b}
        else:
            spans = [(name, span) for name, (_, span) in fields.items()]
            spans += [c for c in capi.cloud_filter_created_fields(st) if c[0] not in fields]
            if len(spans) > capi.MAX_FIELDS:
                raise NotImplementedError(f"a filter chain carries at most {capi.MAX_FIELDS} descriptors")
            flist = [(name, fields[name][0] if name in fields else None, buf(f"{tag}_{k}_{name}", n * span * 4).value, span)
                     for name, span in spans]
            m = reg.filter_cloud_device(cur, stride, n, st, flist, ox.value, oi.value)
            fields = {name: (out, span) for name, _, out, span in flist}
        idx_stages.append((f"{tag}_{k}_idx", m))
        cur, stride, n = ox.value, 3, m
    return cur, stride, n, fields, idx_stages


def _chain_filter(f):
    """One yaml entry of a chain applied outside loadFromYaml: everything _reading_filter binds, and VoxelGrid."""
    name, args = _split(f)
    if name == "VoxelGridDataPointsFilter":
        return VoxelGridDataPointsFilter(**args)
    return _reading_filter(f)


def parse_filters(chain) -> list:
    """A yaml list of data-point filters (as under readingDataPointsFilters) -> the parsed chain."""
    return [_chain_filter(f) for f in (chain or [])]


class FilterChainRunner:
    """Keeps one handle and its device buffers across calls: the mapper applies the same chain to every scan, and a
    fresh handle plus fresh allocations per call would cost more than the kernels."""

    def __init__(self):
        self._reg = None
        self._dev = {}

    def _buf(self, key, nbytes):
        b = self._dev.get(key)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self._dev[key] = capi.DeviceArray(nbytes)
        return b

    def apply(self, filters, cloud: DataPoints, return_indices: bool = False):
        parsed = [_chain_filter(f) if isinstance(f, str) or (isinstance(f, dict) and "type" not in f) else f
                  for f in filters]
        _check_fields(parsed, _cloud_fields(cloud))
        if self._reg is None:
            self._reg = capi.Registration(capi.default_params())
        try:
            cur, stride, n, fields, stages = run_filter_chain(self._reg, self._buf, "fc", parsed, cloud)
            xyz = capi.download(cur, (n, stride))[:, :3].copy()
            desc = {name: capi.download(ptr, (n, span)) for name, (ptr, span) in fields.items()}
            idx = None
            for key, m in stages:
                step = self._dev[key].download(m, np.int32)
                idx = step if idx is None else idx[step]
            if idx is None:
                idx = np.arange(n, dtype=np.int32)
        except RegError as e:
            raise _translate(e) from None
        out = DataPoints(xyz, desc.pop("normals", None), desc.pop("covariances", None), desc)
        return (out, idx) if return_indices else out

    def close(self):
        for b in self._dev.values():
            b.free()
        self._dev = {}
        if self._reg is not None:
            self._reg.close()
            self._reg = None


def filter_cloud(filters, cloud: DataPoints, return_indices: bool = False, runner: "FilterChainRunner | None" = None):
    """Applies a chain (parse_filters' output, or the yaml list itself) to a cloud on the device, outside a registration:
    `icp.readingDataPointsFilters.apply(cloud)` of the reference.  Returns the filtered DataPoints (features m x 3), with
    return_indices also the source index of every kept point.  Pass a FilterChainRunner to keep the handle and the
    device buffers between calls (one per scan stream); without one they live for this call only."""
    own = runner is None
    r = FilterChainRunner() if own else runner
    try:
        return r.apply(filters, cloud, return_indices)
    finally:
        if own:
            r.close()


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
        self.epsilon_ = 1e-3            # TransformationEstimationForGeneralizedICP's default
        self._reg = None

    def params(self) -> RegParams:
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
        return p

    @staticmethod
    def _needs_covariances(cloud: DataPoints) -> bool:
        return cloud.covariances is None and cloud.normals is not None

    def _set(self, reg, cloud: DataPoints, setter32, setter64):
        """A cloud with covariances goes in as before; one with normals only gets the covariances Open3D's GeneralizedICP
        derives from them (reg_covariances_from_normals, epsilon_), as the reference's clouds do."""
        if not self._needs_covariances(cloud):
            return setter32(cloud.features, None, cloud.covariances)
        x = _xyz64(cloud, "cloud")
        covs = reg.covariances_from_normals(_field64(cloud.normals, x.shape[0], 3, "normals"), self.epsilon_)
        return setter64(x, None, covs)

    def registerClouds(self, source: DataPoints, target: DataPoints, init=None) -> RegistrationResult:
        reg = capi.Registration(self.params())
        try:
            self._set(reg, target, reg.set_target, reg.set_target_f64)
            self._set(reg, source, reg.set_source, reg.set_source_f64)
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


# ---- submap-pair constraints (constraint_builders.cpp:43-90, PlaceRecognition.cpp:97-149) ----------------------
ICP_RUN_UNTIL_CONVERGENCE_ITERATIONS = 100   # magic::icpRunUntilConvergenceNumberOfIterations (constraint_builders.cpp:63)


@dataclass
class Constraint:
    """o3d_slam::Constraint, the fields the two builders fill (constraint_builders.cpp:75-82, PlaceRecognition.cpp:140-150)."""
    sourceSubmapIdx_: int = 0
    targetSubmapIdx_: int = 0
    sourceToTarget_: np.ndarray = field(default_factory=lambda: np.eye(4))
    informationMatrix_: np.ndarray = field(default_factory=lambda: np.eye(6))
    isInformationMatrixValid_: bool = False
    isOdometryConstraint_: bool = False


def _xyz64(cloud, what):
    a = np.asarray(cloud.features if isinstance(cloud, DataPoints) else cloud)
    if a.ndim != 2 or a.shape[1] not in (3, 4):
        raise InvalidParameter(f"{what}: points must be N x 3 (or N x 4 homogeneous), got shape {a.shape}")
    return np.ascontiguousarray(a[:, :3], np.float64)


def _field64(a, n, width, what):
    if a is None:
        return None
    a = np.asarray(a)
    if a.ndim != 2 or a.shape != (n, width):
        raise InvalidParameter(f"{what} must be {n} x {width}, got shape {a.shape}")
    return np.ascontiguousarray(a, np.float64)


def _covs9(c6):
    """DataPoints.covariances (xx xy xz yy yz zz) -> Open3D's row-major Matrix3d."""
    return None if c6 is None else np.ascontiguousarray(c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]])


def _check_overlap_args(sourceToTarget, voxelSize, minNumPointsPerVoxel):
    if not (isinstance(voxelSize, (int, float, np.floating, np.integer)) and math.isfinite(voxelSize) and voxelSize > 0):
        raise InvalidParameter(f"voxelSize must be finite and > 0, got {voxelSize!r}")
    if not (isinstance(minNumPointsPerVoxel, (int, np.integer)) and not isinstance(minNumPointsPerVoxel, bool)
            and minNumPointsPerVoxel >= 1):
        raise InvalidParameter(f"minNumPointsPerVoxel must be an integer >= 1, got {minNumPointsPerVoxel!r}")   # assert_ge
    if sourceToTarget is None:
        return None
    T = np.asarray(sourceToTarget, np.float64)
    if T.shape != (4, 4):
        raise InvalidParameter(f"sourceToTarget must be 4 x 4, got shape {T.shape}")
    return T


def computeIndicesOfOverlappingPoints(source, target, sourceToTarget, voxelSize, minNumPointsPerVoxel=1):
    """o3d_slam::computeIndicesOfOverlappingPoints (helpers.cpp:320-345) on the device: (idxsSource, idxsTarget), ascending
    (the reference emits std::unordered_map order).  `source` / `target`: DataPoints or N x 3 arrays; sourceToTarget 4 x 4 or
    None (identity)."""
    T = _check_overlap_args(sourceToTarget, voxelSize, minNumPointsPerVoxel)
    s, t = _xyz64(source, "source"), _xyz64(target, "target")
    p = capi.default_params()
    p.cost = capi.COST_O3D_P2P
    reg = capi.Registration(p)
    try:
        return reg.overlap_indices(s, t, voxelSize, T, minNumPointsPerVoxel)
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()


def _pair_on_handle(reg, source, target, T, voxelSize, needs_target_normals, needs_covs):
    """One upload per cloud: the overlap front (voxelSize not None) or the plain fp64 entry points."""
    s, t = _xyz64(source, "source"), _xyz64(target, "target")
    tn = _field64(target.normals, t.shape[0], 3, "target normals") if needs_target_normals else None
    sc = _covs9(_field64(source.covariances, s.shape[0], 6, "source covariances")) if needs_covs else None
    tc = _covs9(_field64(target.covariances, t.shape[0], 6, "target covariances")) if needs_covs else None
    if voxelSize is not None:
        reg.set_pair_overlap_f64(s, t, voxelSize, T, 1, None, sc, tn, tc)
    else:
        reg.set_target_f64(t, tn, tc)
        reg.set_source_f64(s, None, sc)


def _result_of(reg, T, res) -> RegistrationResult:
    ids, _, _ = reg.correspondences(want_w=False)
    sel = np.nonzero(ids >= 0)[0]
    return RegistrationResult(T.astype(np.float64), float(res.fitness), float(res.inlier_rmse),
                              np.stack([sel, ids[sel]], axis=1))


def buildConstraint(source: DataPoints, target: DataPoints, *, isComputeOverlap, icpMaxCorrespondenceDistance,
                    voxelSizeOverlapCompute, isEstimateInformationMatrix, isSkipIcpRefinement, sourceIdx=0, targetIdx=0,
                    withResult=False):
    """o3d_slam::buildConstraint (constraint_builders.cpp:43-90) for two submap clouds: overlap selection at identity
    (minNumPointsPerVoxel = 1), Open3D point-to-plane RegistrationICP from identity with max_iteration_ = 100, the
    information matrix at the result with the same distance -- one handle, one upload per cloud.  With `withResult` the
    RegistrationResult (indices into the selected clouds, as in the reference) is returned next to the Constraint."""
    if isComputeOverlap:
        _check_overlap_args(None, voxelSizeOverlapCompute, 1)
    if not (math.isfinite(icpMaxCorrespondenceDistance) and icpMaxCorrespondenceDistance > 0):
        raise InvalidParameter(f"icpMaxCorrespondenceDistance must be finite and > 0, got {icpMaxCorrespondenceDistance!r}")
    if target.normals is None and not isSkipIcpRefinement:
        raise InvalidField("point-to-plane needs normals on the target cloud")
    op = RegistrationIcpPointToPlane(icpMaxCorrespondenceDistance, ICP_RUN_UNTIL_CONVERGENCE_ITERATIONS)
    has_nrm = target.normals is not None
    p = op.params()
    if not has_nrm:
        p.cost = capi.COST_O3D_P2P   # no refinement asked for: only the search structure and the information matrix are used
    s, t = _xyz64(source, "source"), _xyz64(target, "target")   # shape errors before the device is touched
    _field64(target.normals, t.shape[0], 3, "target normals")
    reg = capi.Registration(p)
    result = RegistrationResult()
    info = np.eye(6)
    try:
        _pair_on_handle(reg, source, target, None, voxelSizeOverlapCompute if isComputeOverlap else None, has_nrm, False)
        if not isSkipIcpRefinement:
            T, res = reg.register(np.eye(4))
            result = _result_of(reg, T, res)
        if isEstimateInformationMatrix:
            info, _ = reg.information_matrix(result.transformation_, icpMaxCorrespondenceDistance)
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()
    c = Constraint(sourceIdx, targetIdx, result.transformation_.copy(), info, bool(isEstimateInformationMatrix), True)
    return (c, result) if withResult else c


def refineLoopClosure(source: DataPoints, target: DataPoints, T_ransac, registration, voxelSizeForOverlap,
                      maxIcpCorrespondenceDistance, sourceIdx=0, targetIdx=0):
    """The refinement of a loop-closure candidate (PlaceRecognition.cpp:97-149): overlap selection at T_ransac
    (minNumPointsPerVoxel = 1), the given B1 operator from T_ransac on the overlap clouds, the information matrix on the same
    clouds at the refined pose.  Returns (Constraint, RegistrationResult): the caller applies minRefinementFitness_ and the
    consistency check.  maxIcpCorrespondenceDistance must not exceed the operator's maxCorrespondenceDistance_ (the reach of
    the search structure both run on)."""
    T0 = _check_overlap_args(T_ransac, voxelSizeForOverlap, 1)
    if T0 is None:
        T0 = np.eye(4)
    if not (0 < maxIcpCorrespondenceDistance <= registration.maxCorrespondenceDistance_):
        raise InvalidParameter("maxIcpCorrespondenceDistance must be > 0 and <= the operator's maxCorrespondenceDistance_")
    p = registration.params()
    needs_nrm = p.cost == capi.COST_O3D_P2PL
    needs_cov = p.cost == capi.COST_GICP
    if needs_nrm and target.normals is None:
        raise InvalidField("point-to-plane needs normals on the target cloud")
    if needs_cov and (source.covariances is None or target.covariances is None):
        raise InvalidField("GICP needs covariances on both clouds")
    s, t = _xyz64(source, "source"), _xyz64(target, "target")
    if needs_nrm:
        _field64(target.normals, t.shape[0], 3, "target normals")
    reg = capi.Registration(p)
    try:
        _pair_on_handle(reg, source, target, T0, voxelSizeForOverlap, needs_nrm, needs_cov)
        T, res = reg.register(T0)
        result = _result_of(reg, T, res)
        info, _ = reg.information_matrix(result.transformation_, maxIcpCorrespondenceDistance)
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()
    return Constraint(sourceIdx, targetIdx, result.transformation_.copy(), info, True, False), result


# ---- FPFH features and feature matching: the front of place recognition (Submap.cpp:255-275, PlaceRecognition.cpp:71-85;
#      DESIGN.md 5p; PARITY UNPINNED against Open3D 0.15.1) ----------------------------------------------------------------------
@dataclass
class Feature:
    """open3d::pipelines::registration::Feature: `data_` is 33 x n float64, one column per point."""
    data_: np.ndarray = field(default_factory=lambda: np.zeros((33, 0)))

    def Dimension(self) -> int:
        return int(self.data_.shape[0])

    def Num(self) -> int:
        return int(self.data_.shape[1])


@dataclass
class PlaceRecognitionParameters:
    """o3d_slam::PlaceRecognitionParameters: the fields Submap::computeFeatures reads (Parameters.hpp:121-126), then the
    RANSAC fields of PlaceRecognition.cpp:78-91 (Parameters.hpp:127-133)."""
    normalEstimationRadius_: float = 1.0
    featureVoxelSize_: float = 0.5
    featureRadius_: float = 2.5
    featureKnn_: int = 100
    normalKnn_: int = 10
    ransacNumIter_: int = 1000000
    ransacProbability_: float = 0.99
    ransacModelSize_: int = 3
    ransacMaxCorrespondenceDistance_: float = 0.75
    correspondenceCheckerDistance_: float = 0.75
    correspondenceCheckerEdgeLength_: float = 0.5
    ransacMinCorrespondenceSetSize_: int = 25


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_fpfh_args(radius, max_nn):
    if not (isinstance(radius, (int, float, np.floating, np.integer)) and math.isfinite(radius) and radius > 0):
        raise InvalidParameter(f"radius must be finite and > 0, got {radius!r}")
    if not (_is_int(max_nn) and 2 <= max_nn <= 128):
        raise InvalidParameter(f"max_nn must be an integer in [2, 128], got {max_nn!r}")


def _feature_handle():
    p = capi.default_params()
    p.cost = capi.COST_O3D_P2P
    return capi.Registration(p)


def ComputeFPFHFeature(cloud: DataPoints, radius, max_nn=100) -> Feature:
    """ComputeFPFHFeature(cloud, KDTreeSearchParamHybrid(radius, max_nn)) on the device (reg_compute_fpfh).  The cloud needs
    the `normals` descriptor."""
    _check_fpfh_args(radius, max_nn)
    if cloud.normals is None:
        raise InvalidField("FPFH needs normals on the cloud")
    x = np.asarray(cloud.features)
    if x.ndim != 2 or x.shape[1] not in (3, 4):
        raise InvalidParameter(f"points must be N x 3 (or N x 4 homogeneous), got shape {x.shape}")
    nr = np.asarray(cloud.normals)
    if nr.ndim != 2 or nr.shape[0] != x.shape[0] or nr.shape[1] < 3:
        raise InvalidParameter(f"normals must be {x.shape[0]} x 3, got shape {nr.shape}")
    reg = _feature_handle()
    try:
        out = reg.compute_fpfh(x, nr, radius, max_nn)
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()
    return Feature(np.ascontiguousarray(out["fpfh"].T))


def _feature_rows(f, what):
    d = np.asarray(f.data_ if isinstance(f, Feature) else f, np.float64)
    if d.ndim != 2 or not (1 <= d.shape[0] <= 64):
        raise InvalidParameter(f"{what}: data_ must be dim x n with 1 <= dim <= 64, got shape {d.shape}")
    return np.ascontiguousarray(d.T)


def CorrespondencesFromFeatures(source_feature, target_feature, mutual_filter=True, ransac_n=3) -> np.ndarray:
    """The correspondence set RegistrationRANSACBasedOnFeatureMatching forms before it samples: (n, 2) int32 pairs
    (source, target).  With mutual_filter the mutual nearest neighbours when there are at least ransac_n of them, else --
    as Open3D falls back -- every (a, nearest b)."""
    if not (_is_int(ransac_n) and ransac_n >= 1):
        raise InvalidParameter(f"ransac_n must be an integer >= 1, got {ransac_n!r}")
    a, b = _feature_rows(source_feature, "source_feature"), _feature_rows(target_feature, "target_feature")
    if a.shape[1] != b.shape[1]:
        raise InvalidParameter(f"the features have different dimensions ({a.shape[1]} and {b.shape[1]})")
    reg = _feature_handle()
    try:
        nn_ab, _, mutual = reg.match_features(a, b, backward=bool(mutual_filter), mutual=bool(mutual_filter))
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()
    if mutual_filter and mutual.shape[0] >= ransac_n:
        return mutual
    return np.stack([np.arange(nn_ab.size, dtype=np.int32), nn_ab], axis=1)


def computeSubmapFeatures(cloud_f64, params: "PlaceRecognitionParameters | None" = None):
    """o3d_slam::Submap::computeFeatures (Submap.cpp:255-275) on one handle: voxel down-sampling of the whole fp64 cloud at
    featureVoxelSize_ (reg_voxelize_within_volume), normals by hybrid search (normalKnn_, normalEstimationRadius_) oriented
    towards the origin (reg_estimate_normals), FPFH (featureRadius_, featureKnn_).  Returns (DataPoints, Feature): the
    sparse cloud with its normals, and its features.
    Deviation: the voxel grid starts at 0, not at Open3D's min_bound - voxel/2, and the voxels come in ascending (z, y, x)
    index order, where VoxelDownSample emits them in hash-map order."""
    prm = params if params is not None else PlaceRecognitionParameters()
    _check_fpfh_args(prm.featureRadius_, prm.featureKnn_)
    _check_overlap_args(None, prm.featureVoxelSize_, 1)
    if not (_is_int(prm.normalKnn_) and 1 <= prm.normalKnn_ <= 32):
        raise InvalidParameter(f"normalKnn_ must be an integer in [1, 32], got {prm.normalKnn_!r}")
    if not (prm.normalEstimationRadius_ > 0):
        raise InvalidParameter(f"normalEstimationRadius_ must be > 0, got {prm.normalEstimationRadius_!r}")
    x = _xyz64(cloud_f64, "cloud")
    reg = _feature_handle()
    try:
        sparse, _, _, _ = reg.voxelize_within_volume(x, prm.featureVoxelSize_)
        pts = sparse.astype(np.float32)
        nrm = reg.estimate_normals(pts, k=prm.normalKnn_, max_dist=prm.normalEstimationRadius_,
                                   viewpoint=np.zeros(3, np.float32))["normals"]
        out = reg.compute_fpfh(pts, nrm, prm.featureRadius_, prm.featureKnn_)
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()
    return DataPoints(pts, normals=nrm), Feature(np.ascontiguousarray(out["fpfh"].T))


# ---- the scan front end: VoxelDownSample, RandomDownSample, processForScanMatchingAndMerging (ScanToMapRegistration.cpp:36-69;
#      DESIGN.md 5r; PARITY UNPINNED against Open3D 0.15.1) ------------------------------------------------------------------
@dataclass
class PointCloud:
    """The fields of open3d::geometry::PointCloud the front end and the dense map touch: points_ / normals_ n x 3,
    covariances_ n x 9 (row-major Matrix3d), colors_ n x 3, all float64."""
    points_: np.ndarray
    normals_: np.ndarray | None = None
    covariances_: np.ndarray | None = None
    colors_: np.ndarray | None = None

    def HasNormals(self) -> bool:
        return self.normals_ is not None

    def HasCovariances(self) -> bool:
        return self.covariances_ is not None

    def HasColors(self) -> bool:
        return self.colors_ is not None


@dataclass
class DeviceCloud:
    """A cloud resident in HBM: torch float64 tensors (points_ >= n x 3, normals_ / covariances_ >= n x 3 / n x 9 or None)
    of which the first n rows count.  The tensors keep the memory alive."""
    points_: object
    normals_: object = None
    covariances_: object = None
    n: int = 0


@dataclass
class ProcessedScans:
    """o3d_slam::ProcessedScans (ScanToMapRegistration.hpp): the narrow-cropped cloud that is matched, the wide one that is merged."""
    match_: PointCloud
    merge_: PointCloud


def _cloud64(cloud, what="cloud") -> PointCloud:
    """PointCloud, DataPoints (covariances N x 6) or a bare N x 3 array -> validated contiguous float64 arrays."""
    if isinstance(cloud, PointCloud):
        x = np.asarray(cloud.points_)
        if x.ndim != 2 or x.shape[1] != 3:
            raise InvalidParameter(f"{what}: points_ must be N x 3, got shape {x.shape}")
        x = np.ascontiguousarray(x, np.float64)
        cv = cloud.covariances_
        if cv is not None:
            cv = np.asarray(cv)
            if cv.shape == (x.shape[0], 3, 3):
                cv = cv.reshape(-1, 9)
        return PointCloud(x, _field64(cloud.normals_, x.shape[0], 3, f"{what}: normals_"),
                          _field64(cv, x.shape[0], 9, f"{what}: covariances_"),
                          _field64(cloud.colors_, x.shape[0], 3, f"{what}: colors_"))
    if isinstance(cloud, DataPoints):
        x = _xyz64(cloud, what)
        return PointCloud(x, _field64(cloud.normals, x.shape[0], 3, f"{what}: normals"),
                          _covs9(_field64(cloud.covariances, x.shape[0], 6, f"{what}: covariances")))
    return PointCloud(_xyz64(cloud, what))


def _check_voxel_size(voxel_size):
    if not (_is_real(voxel_size) and math.isfinite(voxel_size) and voxel_size > 0):
        raise InvalidParameter(f"voxel_size must be finite and > 0, got {voxel_size!r}")   # Open3D: "voxel_size <= 0."


def _check_ratio_seed(ratio, seed):
    if not (_is_real(ratio) and 0.0 <= ratio <= 1.0):
        raise InvalidParameter(f"sampling_ratio must lie in [0, 1], got {ratio!r}")
    if not (_is_int(seed) and 0 <= seed < 2 ** 64):
        raise InvalidParameter(f"seed must be an integer in [0, 2^64), got {seed!r}")


def VoxelDownSample(cloud, voxel_size) -> PointCloud:
    """PointCloud::VoxelDownSample(voxel_size) on the device (reg_voxel_down_sample): the grid starts at min_bound -
    voxel_size / 2, averaged normals are not re-normalised.  Deviation: the voxels come in ascending (z, y, x) index order,
    where Open3D emits them in hash-map order."""
    _check_voxel_size(voxel_size)
    c = _cloud64(cloud)
    reg = _feature_handle()
    try:
        return PointCloud(*reg.voxel_down_sample(c.points_, voxel_size, c.normals_, c.covariances_))
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()


def RandomDownSample(cloud, sampling_ratio, seed=0) -> PointCloud:
    """PointCloud::RandomDownSample(sampling_ratio) on the device (reg_random_down_sample).  Deviation: Open3D seeds an
    mt19937 from std::random_device; here the kept set is a function of (n, sampling_ratio, seed) only."""
    _check_ratio_seed(sampling_ratio, seed)
    c = _cloud64(cloud)
    reg = _feature_handle()
    try:
        _, x, nr, cv = reg.random_down_sample(c.points_.shape[0], sampling_ratio, seed, c.points_, c.normals_, c.covariances_)
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()
    return PointCloud(x, nr, cv)


class ScanToMapIcp:
    """o3d_slam::ScanToMapIcp's scan side (ScanToMapRegistration.cpp:25-69) on one handle: processForScanMatchingAndMerging
    runs the whole front end on the device (reg_process_scan) and leaves match_ installed as the reading of `icp`'s handle,
    so that register() -- or any entry point that uses the current reading -- follows without an upload.
    `icp`: a configured ICP / PointMatcherICP (default: ICP with the shipped parameters); the croppers are the crop dicts of
    capi.Registration.set_target_f64 (None: no cropping); knn_ 0 turns the normal estimation off."""

    def __init__(self, icp: "ICP | None" = None, *, mapBuilderCropper=None, scanMatcherCropper=None, voxelSize_=0.01,
                 downSamplingRatio_=1.0, knn_=20, maxDistanceKnn_=1.0, seed=0):
        if icp is None:
            icp = ICP()
            icp.params = capi.shipped_params()
        self.icp = icp
        self.mapBuilderCropper, self.scanMatcherCropper = mapBuilderCropper, scanMatcherCropper
        self.voxelSize_, self.downSamplingRatio_ = voxelSize_, downSamplingRatio_
        self.knn_, self.maxDistanceKnn_, self.seed = knn_, maxDistanceKnn_, seed
        self.last_scan = None

    def _check(self):
        if not (_is_real(self.voxelSize_) and math.isfinite(self.voxelSize_)):     # <= 0 skips the stage (helpers.cpp:108-111)
            raise InvalidParameter(f"voxelSize_ must be finite, got {self.voxelSize_!r}")
        if not (_is_real(self.downSamplingRatio_) and math.isfinite(self.downSamplingRatio_) and self.downSamplingRatio_ >= 0):
            raise InvalidParameter(f"downSamplingRatio_ must be finite and >= 0, got {self.downSamplingRatio_!r}")
        _check_ratio_seed(0.0, self.seed)
        if not (_is_int(self.knn_) and 0 <= self.knn_ <= 32):
            raise InvalidParameter(f"knn_ must be an integer in [0, 32], got {self.knn_!r}")
        if self.knn_ > 0 and not (_is_real(self.maxDistanceKnn_) and self.maxDistanceKnn_ > 0):
            raise InvalidParameter(f"maxDistanceKnn_ must be > 0, got {self.maxDistanceKnn_!r}")   # assert_gt
        for name in ("mapBuilderCropper", "scanMatcherCropper"):
            crop = getattr(self, name)
            if crop is not None and not (isinstance(crop, dict) and crop.get("type", 0) in (0, 1, 2, 3, 4)):
                raise InvalidParameter(f"{name} must be a crop dict with a known type, got {crop!r}")

    def processForScanMatchingAndMerging(self, cloud) -> ProcessedScans:
        self._check()
        c = _cloud64(cloud, "scan")
        if c.points_.shape[0] == 0:
            raise RuntimeError("The reading point cloud is empty.")
        self.icp._ensure()
        prm = capi.default_scan_params(wide=self.mapBuilderCropper, narrow=self.scanMatcherCropper,
                                       voxel_size=float(self.voxelSize_), down_sampling_ratio=float(self.downSamplingRatio_),
                                       seed=int(self.seed), normal_knn=int(self.knn_),
                                       normal_radius=float(self.maxDistanceKnn_) if self.knn_ > 0 else 1.0)
        reg = self.icp._reg
        try:
            x, nr, cv, res = reg.process_scan(c.points_, prm, c.normals_, c.covariances_)
            idx = reg.source_source_indices()
        except RegError as e:
            raise _translate(e) from None
        self.last_scan = res
        pick = lambda a: a[idx] if a is not None else None
        return ProcessedScans(PointCloud(x[idx], pick(nr), pick(cv)), PointCloud(x, nr, cv))

    def processForScanMatchingAndMergingDevice(self, cloud) -> "DeviceCloud":
        """As processForScanMatchingAndMerging, with merge_ left in device arrays (torch tensors) and no host copy of it:
        the DeviceCloud goes straight into Submap.insertScan.  match_ is the reading installed on the handle."""
        import torch
        self._check()
        c = _cloud64(cloud, "scan")
        n = c.points_.shape[0]
        if n == 0:
            raise RuntimeError("The reading point cloud is empty.")
        self.icp._ensure()
        prm = capi.default_scan_params(wide=self.mapBuilderCropper, narrow=self.scanMatcherCropper,
                                       voxel_size=float(self.voxelSize_), down_sampling_ratio=float(self.downSamplingRatio_),
                                       seed=int(self.seed), normal_knn=int(self.knn_),
                                       normal_radius=float(self.maxDistanceKnn_) if self.knn_ > 0 else 1.0)
        dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda") if a is not None else None
        x, nr, cv = dev(c.points_), dev(c.normals_), dev(c.covariances_)
        ox, on, oc = (torch.empty((n, w), dtype=torch.float64, device="cuda") for w in (3, 3, 9))
        ptr = lambda t: t.data_ptr() if t is not None else None
        try:
            res = self.icp._reg.process_scan_device(ptr(x), n, prm, ptr(ox), ptr(nr), ptr(cv), ptr(on), ptr(oc))
        except RegError as e:
            raise _translate(e) from None
        self.last_scan = res
        return DeviceCloud(ox, on if res.has_normals else None, oc if res.has_covs else None, int(res.n_merge))

    def register(self, T_init=None):
        """ICP::compute on the reading processForScanMatchingAndMerging left on the handle: (T, result)."""
        try:
            T, res = self.icp._reg.register(np.eye(4, dtype=np.float32) if T_init is None else T_init)
        except RegError as e:
            raise _translate(e) from None
        self.icp.last_result = res
        return T, res


# ---- the dense map: VoxelizedPointCloud, ColorRangeCropper, space carving, Submap::insertScanDenseMap (Voxel.cpp:38-191,
#      croppers.cpp:178-239, helpers.cpp:360-402, Submap.cpp:98-113,146-157) ------------------------------------
def _check_T(T, what):
    if T is None:
        return None
    T = np.asarray(T, np.float64)
    if T.shape != (4, 4):
        raise InvalidParameter(f"{what} must be 4 x 4, got shape {T.shape}")
    return T


@dataclass
class SpaceCarvingParameters:
    """o3d_slam::SpaceCarvingParameters (Parameters.hpp:88-95): the fields the dense map reads."""
    maxRaytracingLength_: float = 20.0
    truncationDistance_: float = 0.1
    carveSpaceEveryNscans_: int = 10
    neighborhoodRadiusDenseMap_: float = 0.1
    voxelSize_: float = 0.1                    # the two fields only the first map's carve reads (icp.Submap)
    minDotProductWithNormal_: float = 0.5

    def check(self, voxelSize):
        r, mr, tr = self.neighborhoodRadiusDenseMap_, self.maxRaytracingLength_, self.truncationDistance_
        if not (_is_real(r) and math.isfinite(r) and r > 0 and _is_real(mr) and math.isfinite(mr) and mr > 0
                and _is_real(tr) and math.isfinite(tr)):
            raise InvalidParameter("carving: neighborhoodRadiusDenseMap_ and maxRaytracingLength_ must be finite and > 0, "
                                   "truncationDistance_ finite (the reference loops forever at a radius <= 0)")
        if not (_is_int(self.carveSpaceEveryNscans_) and self.carveSpaceEveryNscans_ >= 1):
            raise InvalidParameter(f"carveSpaceEveryNscans_ must be an integer >= 1, got {self.carveSpaceEveryNscans_!r}")
        n, d = 0, -float(r)
        while d <= r:                     # the running sum of VoxelHashMap.cpp:25-27
            n, d = n + 1, d + float(voxelSize)
            if n > 16:
                raise InvalidParameter("carving: more than 16 neighbourhood offsets per axis (radius / voxel size too large)")
        if mr / (2.0 * r) > 65536.0:
            raise InvalidParameter("carving: maxRaytracingLength_ / (2 neighborhoodRadiusDenseMap_) must not exceed 65536")

    def params(self) -> "capi.DenseCarveParams":
        return capi.default_dense_carve_params(neighborhood_radius=self.neighborhoodRadiusDenseMap_,
                                               max_ray=self.maxRaytracingLength_, truncation=self.truncationDistance_)


class ColorRangeCropper:
    """o3d_slam::ColorRangeCropper (croppers.cpp:178-239): keeps rgbMin <= c <= rgbMax on every channel; a cloud without
    colours passes whole.  On the device it is one stage of DenseMapBuilder.insertScanDenseMap (reg_dense_map_insert_scan);
    getIndicesWithValidColor / crop here are the host-side views of the same rule for callers that hold numpy clouds."""

    def __init__(self, rgbMin=(0.0, 0.0, 0.0), rgbMax=(1.0, 1.0, 1.0)):
        self.setMinBounds(rgbMin)
        self.setMaxBounds(rgbMax)

    @staticmethod
    def _bound(v, what):
        try:
            a = np.asarray(v, np.float64)
        except (TypeError, ValueError):
            a = np.zeros(0)
        if a.shape != (3,) or np.isnan(a).any():
            raise InvalidParameter(f"{what} must be three numbers, got {v!r}")
        return a

    def setMinBounds(self, rgbMin):
        self.rgbMin_ = self._bound(rgbMin, "rgbMin")

    def setMaxBounds(self, rgbMax):
        self.rgbMax_ = self._bound(rgbMax, "rgbMax")

    def isValidColor(self, c) -> bool:
        c = np.asarray(c, np.float64)
        return bool(np.all(self.rgbMin_ <= c) and np.all(c <= self.rgbMax_))

    def getIndicesWithValidColor(self, cloud) -> np.ndarray:
        c = _cloud64(cloud)
        if not c.HasColors():
            return np.arange(c.points_.shape[0])
        return np.nonzero(np.all((self.rgbMin_ <= c.colors_) & (c.colors_ <= self.rgbMax_), axis=1))[0]

    def crop(self, cloud) -> PointCloud:
        c = _cloud64(cloud)
        if not c.HasColors():
            return c
        idx = self.getIndicesWithValidColor(c)
        pick = lambda a: a[idx] if a is not None else None
        return PointCloud(c.points_[idx], pick(c.normals_), pick(c.covariances_), c.colors_[idx])


class VoxelizedPointCloud:
    """o3d_slam::VoxelizedPointCloud (Voxel.cpp:38-114) resident on the device (capi.DenseMap): per-voxel running sums of
    positions, normals and colours.  `reg`: the capi.Registration whose stream and working storage the map uses (default:
    a handle of its own).  Departures: toPointCloud emits the voxels in ascending (z, y, x) key order (the reference: hash-map
    order); a non-finite point or a voxel index outside +-(2^20 - 1) raises InvalidParameter and leaves the map unchanged.
    transform reproduces the reference literally: it maps every position and normal SUM by R S + t and keeps the keys,
    which is wrong for any t != 0."""

    def __init__(self, voxelSize=0.25, reg: "capi.Registration | None" = None):
        _check_voxel_size(voxelSize)
        self._own = reg is None
        self._reg = reg if reg is not None else _feature_handle()
        self.map = capi.DenseMap(self._reg, voxelSize)
        self.voxelSize_ = float(voxelSize)

    def close(self):
        self.map.close()
        if self._own:
            self._reg.close()

    def getVoxelSize(self) -> float:
        return self.voxelSize_

    def insert(self, cloud, T=None):
        """VoxelizedPointCloud::insert(transform(T, cloud)) (T None: the cloud as it is).  Returns (n_voxels, n_new)."""
        c = _cloud64(cloud)
        try:
            return self.map.insert(c.points_, c.normals_, c.colors_, _check_T(T, "T"))
        except RegError as e:
            raise _translate(e) from None

    def transform(self, T):
        try:
            self.map.transform(_check_T(np.eye(4) if T is None else T, "T"))
        except RegError as e:
            raise _translate(e) from None

    def toPointCloud(self) -> PointCloud:
        e = self.map.export(want_keys=False, want_counts=False)
        return PointCloud(e["xyz"], e["normals"], None, e["colors"])

    def size(self) -> int:
        return int(self.map.info().n_voxels)

    def empty(self) -> bool:
        return self.size() == 0

    def clear(self):
        self.map.clear()

    def hasColors(self) -> bool:
        return bool(self.map.info().has_colors)

    def hasNormals(self) -> bool:
        return bool(self.map.info().has_normals)

    def computeCenter(self) -> np.ndarray:
        """o3d_slam::computeCenter (helpers.cpp:392-402)."""
        return self.map.center()


def removeDuplicatePointsWithinSameVoxels(cloud, voxelSize, reg: "capi.Registration | None" = None) -> PointCloud:
    """o3d_slam::removeDuplicatePointsWithinSameVoxels (Voxel.cpp:162-191) on the device (reg_dedup_voxels): the first point of
    every voxel, in input order, with its normal and colour."""
    _check_voxel_size(voxelSize)
    c = _cloud64(cloud)
    own = reg is None
    reg = _feature_handle() if own else reg
    try:
        idx = reg.dedup_voxels(c.points_, voxelSize)
    except RegError as e:
        raise _translate(e) from None
    finally:
        if own:
            reg.close()
    pick = lambda a: a[idx] if a is not None else None
    return PointCloud(c.points_[idx], pick(c.normals_), pick(c.covariances_), pick(c.colors_))


def getKeysOfCarvedPoints(scan, cloud: VoxelizedPointCloud, sensorPosition, param: "SpaceCarvingParameters | None" = None):
    """o3d_slam::getKeysOfCarvedPoints (helpers.cpp:360-390) on the device, TOGETHER WITH the removeKey loop its only caller
    runs on the result (Submap.cpp:153-156): the voxels are erased from `cloud` by the same call.  Returns their keys,
    k x 3 int32 (x, y, z), in ascending (z, y, x) order (the reference: hash-set order)."""
    param = param if param is not None else SpaceCarvingParameters()
    param.check(cloud.voxelSize_)
    s = np.asarray(sensorPosition, np.float64)
    if s.shape != (3,):
        raise InvalidParameter(f"sensorPosition must be three numbers, got shape {s.shape}")
    try:
        return cloud.map.carve(_cloud64(scan, "scan").points_, s, param.params())
    except RegError as e:
        raise _translate(e) from None


class DenseMapBuilder:
    """The dense-map half of o3d_slam::Submap: insertScanDenseMap (Submap.cpp:98-113) and carve (Submap.cpp:146-157) on
    one device-resident map.  Per scan: dense-map cropper (a crop dict of capi.Registration.set_target_f64, at the pose the
    caller gives it -- the reference sets identity), ColorRangeCropper, transform by mapToRangeSensor, insert -- one call,
    reg_dense_map_insert_scan -- then, when nScansInsertedDenseMap_ % carveSpaceEveryNscans_ == 1 and the map is not empty,
    the carve on the de-duplicated scan.

    Oddity reproduced: the reference carves with the RAW, untransformed scan (sensor frame) against the map-frame sensor
    position mapToRangeSensor.translation(); that is the default here.  carveInMapFrame=True transforms the scan first, which
    is what the geometry asks for."""

    def __init__(self, voxelSize=0.03, cropper=None, colorCropper: "ColorRangeCropper | None" = None,
                 carving: "SpaceCarvingParameters | None" = None, carveInMapFrame=False, reg: "capi.Registration | None" = None):
        self.carving_ = carving if carving is not None else SpaceCarvingParameters()
        self.carving_.check(voxelSize)
        if cropper is not None and not (isinstance(cropper, dict) and cropper.get("type", 0) in (0, 1, 2, 3, 4)):
            raise InvalidParameter(f"cropper must be a crop dict with a known type, got {cropper!r}")
        self.denseMap_ = VoxelizedPointCloud(voxelSize, reg)
        self.denseMapCropper_ = cropper
        self.colorCropper_ = colorCropper if colorCropper is not None else ColorRangeCropper()
        self.carveInMapFrame = bool(carveInMapFrame)
        self.nScansInsertedDenseMap_ = 0
        self.lastCarvedKeys_ = None

    def close(self):
        self.denseMap_.close()

    def insertScanDenseMap(self, rawScan, mapToRangeSensor, isPerformCarving=True) -> bool:
        T = _check_T(mapToRangeSensor, "mapToRangeSensor")
        if T is None:
            raise InvalidParameter("mapToRangeSensor is missing")
        c = _cloud64(rawScan, "rawScan")
        prm = capi.default_dense_scan_params(self.denseMapCropper_, self.colorCropper_.rgbMin_, self.colorCropper_.rgbMax_)
        try:
            self.denseMap_.map.insert_scan(c.points_, prm, c.normals_, c.colors_, T)
        except RegError as e:
            raise _translate(e) from None
        self.lastCarvedKeys_ = None
        if isPerformCarving:
            self.carve(c, T)
        self.nScansInsertedDenseMap_ += 1
        return True

    def carve(self, scan: PointCloud, mapToRangeSensor):
        """Submap::carve for the dense map (Submap.cpp:146-157)."""
        if self.denseMap_.empty() or not (self.nScansInsertedDenseMap_ % self.carving_.carveSpaceEveryNscans_ == 1):
            return
        try:                              # transform, de-duplication, carve and erase in one call (reg_dense_map_carve_scan)
            self.lastCarvedKeys_ = self.denseMap_.map.carve_scan(scan.points_, mapToRangeSensor[:3, 3], self.carving_.params(),
                                                                 mapToRangeSensor if self.carveInMapFrame else None)
        except RegError as e:
            raise _translate(e) from None


# ---- the first map of a submap: Submap::insertScan / carve / transform, cropSubmap + initReference (Submap.cpp:39-144,
#      ScanToMapRegistration.cpp:90-96) -------------------------------------------------------------------------
def _check_crop(crop, what):
    if crop is not None and not (isinstance(crop, dict) and crop.get("type", 0) in (0, 1, 2, 3, 4)):
        raise InvalidParameter(f"{what} must be a crop dict with a known type, got {crop!r}")


class Submap:
    """The scan-matching half of o3d_slam::Submap on one device-resident map cloud (capi.MapCloud): insertScan
    (Submap.cpp:39-96), transform, computeSubmapCenter, getMapPointCloud, and setAsReference = cropSubmap + initReference on
    the same handle.  Built from a ScanToMapIcp it shares that object's handle and map builder cropper, so that
    processForScanMatchingAndMergingDevice -> register -> insertScan -> setAsReference never passes a cloud through the host.
    Otherwise `reg` is the capi.Registration to live on (default: a handle of its own).

    Followed from the reference: the carve runs when nScansInsertedMap_ % carveSpaceEveryNscans_ == 1 (never at 1, never on
    the first insert) and uses the cropper pose of the PREVIOUS insert.  Departure: the field set (normals, covariances) is
    fixed at construction and a scan with other fields raises InvalidParameter (Open3D's operator+= drops the field)."""

    def __init__(self, scanToMap: "ScanToMapIcp | None" = None, *, reg: "capi.Registration | None" = None, mapVoxelSize_=0.03,
                 mapBuilderCropper=None, carving: "SpaceCarvingParameters | None" = None, hasNormals=True, hasCovariances=False,
                 isUseInitialMap_=False, isCarvingEnabled_=True):
        c = carving if carving is not None else SpaceCarvingParameters()
        if not (_is_real(mapVoxelSize_) and not math.isnan(mapVoxelSize_)):
            raise InvalidParameter(f"mapVoxelSize_ must be a number, got {mapVoxelSize_!r}")
        if not (_is_real(c.voxelSize_) and math.isfinite(c.voxelSize_) and c.voxelSize_ > 0):
            raise InvalidParameter(f"carving.voxelSize_ must be finite and > 0, got {c.voxelSize_!r}")
        for name in ("maxRaytracingLength_", "truncationDistance_", "minDotProductWithNormal_"):
            v = getattr(c, name)
            if not (_is_real(v) and not math.isnan(v)):
                raise InvalidParameter(f"carving.{name} must be a number, got {v!r}")
        if not (_is_int(c.carveSpaceEveryNscans_) and c.carveSpaceEveryNscans_ >= 1):
            raise InvalidParameter(f"carveSpaceEveryNscans_ must be an integer >= 1, got {c.carveSpaceEveryNscans_!r}")
        if scanToMap is not None and mapBuilderCropper is None:
            mapBuilderCropper = scanToMap.mapBuilderCropper
        _check_crop(mapBuilderCropper, "mapBuilderCropper")
        self.carving_ = c
        self.isUseInitialMap_, self.isCarvingEnabled_ = bool(isUseInitialMap_), bool(isCarvingEnabled_)
        self.mapVoxelSize_ = float(mapVoxelSize_)
        self._own = scanToMap is None and reg is None
        if scanToMap is not None:
            scanToMap.icp._ensure()
            reg = scanToMap.icp._reg
        self._reg = reg if reg is not None else _feature_handle()
        prm = capi.default_map_cloud_params(mapBuilderCropper if mapBuilderCropper is not None else dict(type=capi.CROP_NONE),
                                            has_normals=bool(hasNormals), has_covariances=bool(hasCovariances),
                                            carve_every_n_scans=c.carveSpaceEveryNscans_, map_voxel_size=self.mapVoxelSize_,
                                            carve_voxel_size=c.voxelSize_, carve_max_ray=c.maxRaytracingLength_,
                                            carve_truncation=c.truncationDistance_, carve_min_dot=c.minDotProductWithNormal_)
        try:
            self.map = capi.MapCloud(self._reg, prm)
        except RegError as e:
            raise _translate(e) from None
        self.lastInsert_ = None

    def close(self):
        self.map.close()
        if self._own:
            self._reg.close()

    @property
    def nScansInsertedMap_(self) -> int:
        return int(self.map.info().scans_inserted)

    @staticmethod
    def _device_args(c):
        ptr = lambda t: t.data_ptr() if t is not None else None
        return ptr(c.points_), ptr(c.normals_), ptr(c.covariances_), int(c.n)

    @staticmethod
    def _to_device(c: PointCloud) -> DeviceCloud:
        import torch
        dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda") if a is not None else None
        return DeviceCloud(dev(c.points_), dev(c.normals_), dev(c.covariances_), c.points_.shape[0])

    def insertScan(self, rawScan, preProcessedScan, mapToRangeSensor, isPerformCarving=True) -> bool:
        """Submap::insertScan.  Either cloud may be a DeviceCloud (then the other is uploaded once); rawScan may be None."""
        T = _check_T(mapToRangeSensor, "mapToRangeSensor")
        if T is None:
            raise InvalidParameter("mapToRangeSensor is missing")
        on_device = isinstance(preProcessedScan, DeviceCloud) or isinstance(rawScan, DeviceCloud)
        scan = preProcessedScan if isinstance(preProcessedScan, DeviceCloud) else _cloud64(preProcessedScan, "preProcessedScan")
        raw = rawScan if rawScan is None or isinstance(rawScan, DeviceCloud) else _cloud64(rawScan, "rawScan")
        n_scan = scan.n if isinstance(scan, DeviceCloud) else scan.points_.shape[0]
        if n_scan == 0:
            return True                                                         # Submap.cpp:41-43
        carve = self.isCarvingEnabled_ and bool(isPerformCarving)
        try:
            if on_device:
                scan = scan if isinstance(scan, DeviceCloud) else self._to_device(scan)
                raw = raw if raw is None or isinstance(raw, DeviceCloud) else self._to_device(raw)
                x, nr, cv, n = self._device_args(scan)
                if self.isUseInitialMap_ and self.map.info().n_rows == 0:       # Submap.cpp:47-52
                    self.map.set_device(x, n, nr, cv, self.mapVoxelSize_)
                    return True
                rp, rn = (raw.points_.data_ptr(), int(raw.n)) if raw is not None else (None, 0)
                self.lastInsert_ = self.map.insert_scan_device(rp, rn, x, n, T, nr, cv, carve)
            else:
                if self.isUseInitialMap_ and self.map.info().n_rows == 0:
                    self.map.set(scan.points_, scan.normals_, scan.covariances_, self.mapVoxelSize_)
                    return True
                self.lastInsert_ = self.map.insert_scan(raw.points_ if raw is not None else None, scan.points_, T, scan.normals_,
                                                        scan.covariances_, carve)
        except RegError as e:
            raise _translate(e) from None
        return True

    def getMapPointCloud(self) -> PointCloud:
        e = self.map.export()
        return PointCloud(e["xyz"], e["normals"], e["covs"])

    def transform(self, T):
        """Submap::transform's mapCloud_.Transform(T)."""
        try:
            self.map.transform(_check_T(np.eye(4) if T is None else T, "T"))
        except RegError as e:
            raise _translate(e) from None

    def computeSubmapCenter(self) -> np.ndarray:
        """mapCloud_.GetCenter() (Submap::computeSubmapCenter)."""
        return self.map.center()

    def setAsReference(self, crop=None) -> int:
        """cropSubmap (scanMatcherCropper_ at its pose: `crop`) + open3dToPointmatcher + initReference from the resident map
        onto the handle.  Returns the rows of the patch; raises as an empty reference does."""
        _check_crop(crop, "crop")
        try:
            return self.map.set_target(crop)
        except RegError as e:
            raise _translate(e) from None


def _transform_points(T, x):
    """o3d_slam::transform's point formula (helpers.cpp:302-303; the contract at reg_overlap_indices), one rounding per
    operation: w = ((T30 x + T31 y) + T32 z) + T33, x' = (((T00 x + T01 y) + T02 z) + T03) / w."""
    w = ((T[3, 0] * x[:, 0] + T[3, 1] * x[:, 1]) + T[3, 2] * x[:, 2]) + T[3, 3]
    return np.stack([(((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3]) / w for r in range(3)], axis=1)


# ---- RANSAC registration on feature correspondences: the hypothesis loop of place recognition (PlaceRecognition.cpp:78-91;
#      DESIGN.md 5q; PARITY UNPINNED against Open3D 0.15.1) ------------------------------------------------------------------
@dataclass
class RANSACConvergenceCriteria:
    """open3d::pipelines::registration::RANSACConvergenceCriteria."""
    max_iteration_: int = 100000
    confidence_: float = 0.999


@dataclass
class CorrespondenceCheckerBasedOnEdgeLength:
    """The sampled edges of source and target must agree in length within similarity_threshold_ (both ways)."""
    similarity_threshold_: float = 0.9


@dataclass
class CorrespondenceCheckerBasedOnDistance:
    """The sampled points must lie within distance_threshold_ of their partners after the fitted transform."""
    distance_threshold_: float


def _is_real(v) -> bool:
    return isinstance(v, (int, float, np.floating, np.integer)) and not isinstance(v, bool)


def _check_ransac_args(max_correspondence_distance, ransac_n, checkers, criteria, seed):
    """Validates and returns (distance_threshold, edge_similarity) of the checkers (0: absent)."""
    if not (_is_real(max_correspondence_distance) and math.isfinite(max_correspondence_distance)
            and max_correspondence_distance > 0):
        raise InvalidParameter(f"max_correspondence_distance must be finite and > 0, got {max_correspondence_distance!r}")
    if not (_is_int(ransac_n) and 3 <= ransac_n <= 8):
        raise InvalidParameter(f"ransac_n must be an integer in [3, 8], got {ransac_n!r}")
    if not isinstance(criteria, RANSACConvergenceCriteria):
        raise InvalidParameter("criteria must be a RANSACConvergenceCriteria")
    if not (_is_int(criteria.max_iteration_) and criteria.max_iteration_ >= 1):
        raise InvalidParameter(f"max_iteration_ must be an integer >= 1, got {criteria.max_iteration_!r}")
    if not (_is_real(criteria.confidence_) and 0.0 <= criteria.confidence_ <= 1.0):
        raise InvalidParameter(f"confidence_ must lie in [0, 1], got {criteria.confidence_!r}")
    if not (_is_int(seed) and 0 <= seed < 2 ** 64):
        raise InvalidParameter(f"seed must be an integer in [0, 2^64), got {seed!r}")
    dist, edge = 0.0, 0.0
    for c in checkers:
        if isinstance(c, CorrespondenceCheckerBasedOnDistance):
            v = c.distance_threshold_
            if not (_is_real(v) and math.isfinite(v) and v > 0) or dist:
                raise InvalidParameter(f"one distance checker with a finite distance_threshold_ > 0, got {v!r}")
            dist = float(v)
        elif isinstance(c, CorrespondenceCheckerBasedOnEdgeLength):
            v = c.similarity_threshold_
            if not (_is_real(v) and 0 < v <= 1) or edge:
                raise InvalidParameter(f"one edge-length checker with similarity_threshold_ in (0, 1], got {v!r}")
            edge = float(v)
        else:
            raise InvalidModuleType(f"unsupported correspondence checker {type(c).__name__} (CorrespondenceCheckerBasedOnNormal "
                                    "is not implemented)")
    return dist, edge


def RegistrationRANSACBasedOnCorrespondence(source, target, corres, max_correspondence_distance, ransac_n=3, checkers=(),
                                            criteria=None, seed=0) -> RegistrationResult:
    """open3d RegistrationRANSACBasedOnCorrespondence with TransformationEstimationPointToPoint(false) on the device
    (reg_ransac_correspondences): `corres` (k, 2) integer pairs (source, target) into the fp64 points of the two clouds.
    Deterministic for a given seed; fewer than ransac_n correspondences, or none that qualifies, give the default result."""
    criteria = RANSACConvergenceCriteria() if criteria is None else criteria
    dist, edge = _check_ransac_args(max_correspondence_distance, ransac_n, tuple(checkers), criteria, seed)
    s, t = _xyz64(source, "source"), _xyz64(target, "target")
    c = np.asarray(corres)
    if c.ndim != 2 or c.shape[1] != 2 or not np.issubdtype(c.dtype, np.integer):
        raise InvalidParameter(f"corres must be k x 2 integers, got shape {c.shape} of {c.dtype}")
    if c.shape[0] == 0:
        return RegistrationResult(correspondence_set_=np.zeros((0, 2), np.int32))
    if c.min() < 0 or c[:, 0].max() >= s.shape[0] or c[:, 1].max() >= t.shape[0]:
        raise InvalidParameter("corres: an index lies outside its cloud")
    reg = _feature_handle()
    try:
        out = reg.ransac_correspondences(s, t, c, max_correspondence_distance, ransac_n, criteria.max_iteration_,
                                         criteria.confidence_, dist, edge, seed)
    except RegError as e:
        raise _translate(e) from None
    finally:
        reg.close()
    return RegistrationResult(out["T"], out["fitness"], out["inlier_rmse"], out["inliers"])


def RegistrationRANSACBasedOnFeatureMatching(source, target, source_feature, target_feature, mutual_filter,
                                             max_correspondence_distance, ransac_n=3, checkers=(), criteria=None,
                                             seed=0) -> RegistrationResult:
    """open3d RegistrationRANSACBasedOnFeatureMatching: CorrespondencesFromFeatures, then
    RegistrationRANSACBasedOnCorrespondence -- both on the device."""
    criteria = RANSACConvergenceCriteria() if criteria is None else criteria
    _check_ransac_args(max_correspondence_distance, ransac_n, tuple(checkers), criteria, seed)
    s, t = _xyz64(source, "source"), _xyz64(target, "target")
    a, b = _feature_rows(source_feature, "source_feature"), _feature_rows(target_feature, "target_feature")
    if a.shape[0] != s.shape[0] or b.shape[0] != t.shape[0]:
        raise InvalidParameter(f"one feature column per point: {a.shape[0]} / {s.shape[0]} and {b.shape[0]} / {t.shape[0]}")
    corres = CorrespondencesFromFeatures(source_feature, target_feature, mutual_filter, ransac_n)
    return RegistrationRANSACBasedOnCorrespondence(s, t, corres, max_correspondence_distance, ransac_n, checkers, criteria,
                                                   seed)


def ransacLoopClosure(sourceSparse, sourceFeature, targetSparse, targetFeature, params=None, seed=0):
    """PlaceRecognition.cpp:78-91: RANSAC on mutually matched features with the edge-length and the distance checker, then
    the size check on the inlier set.  Returns the RegistrationResult, or None when it holds fewer than
    ransacMinCorrespondenceSetSize_ correspondences (the reference skips that candidate)."""
    prm = params if params is not None else PlaceRecognitionParameters()
    if not (_is_int(prm.ransacMinCorrespondenceSetSize_) and prm.ransacMinCorrespondenceSetSize_ >= 0):
        raise InvalidParameter(f"ransacMinCorrespondenceSetSize_ must be an integer >= 0, got "
                               f"{prm.ransacMinCorrespondenceSetSize_!r}")
    for name in ("correspondenceCheckerDistance_", "correspondenceCheckerEdgeLength_"):
        if not _is_real(getattr(prm, name)):
            raise InvalidParameter(f"{name} must be a number, got {getattr(prm, name)!r}")
    result = RegistrationRANSACBasedOnFeatureMatching(
        sourceSparse, targetSparse, sourceFeature, targetFeature, True, prm.ransacMaxCorrespondenceDistance_,
        prm.ransacModelSize_,
        (CorrespondenceCheckerBasedOnEdgeLength(prm.correspondenceCheckerEdgeLength_),
         CorrespondenceCheckerBasedOnDistance(prm.correspondenceCheckerDistance_)),
        RANSACConvergenceCriteria(prm.ransacNumIter_, prm.ransacProbability_), seed)
    if result.correspondence_set_.shape[0] < prm.ransacMinCorrespondenceSetSize_:
        return None
    return result


# ---- motion compensation and the pose buffer it reads (MotionCompensation.cpp, TransformInterpolationBuffer.cpp).
#      Times are integer nanoseconds. ------------------------------------------------------------------------------------------
def _quat_from_R(R):
    """Eigen's Quaterniond(Matrix3d): (w, x, y, z)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([w, (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t])
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q = np.zeros(4)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (R[k, j] - R[j, k]) * t
    q[1 + j] = (R[j, i] + R[i, j]) * t
    q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def _R_from_quat(q):
    """Eigen's toRotationMatrix of (w, x, y, z)."""
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def _slerp(t, a, b):
    """Eigen's QuaternionBase::slerp: the shorter arc, linear when the two nearly coincide."""
    d = float(np.dot(a, b))
    ad = abs(d)
    if ad >= 1.0 - np.finfo(np.float64).eps:
        s0, s1 = 1.0 - t, t
    else:
        theta = math.acos(ad)
        st = math.sin(theta)
        s0, s1 = math.sin((1.0 - t) * theta) / st, math.sin(t * theta) / st
    if d < 0.0:
        s1 = -s1
    return s0 * a + s1 * b


def toRPY(q):
    """o3d_slam::toRPY (math.cpp:39-46, math.hpp:30-42) of (w, x, y, z), normalised first."""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([math.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), math.asin(2 * (w * y - x * z)),
                     math.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))])


def interpolate(start, end, time):
    """o3d_slam::interpolate (Transform.cpp:16-67) of two (time, 4x4) pairs: linear translation, slerp rotation, factor =
    (time - start) / (duration + 1e-6) in seconds; a reversed pair is swapped, a time outside it raises RuntimeError."""
    (t0, T0), (t1, T1) = (start, end) if start[0] <= end[0] else (end, start)
    if time > t1 or time < t0:
        raise RuntimeError("transform interpolate:: query time is not between start and end time")
    factor = ((time - t0) * 1e-9) / ((t1 - t0) * 1e-9 + 1e-6)
    T = np.eye(4)
    T[:3, :3] = _R_from_quat(_slerp(factor, _quat_from_R(T0[:3, :3]), _quat_from_R(T1[:3, :3])))
    T[:3, 3] = T0[:3, 3] + (T1[:3, 3] - T0[:3, 3]) * factor
    return time, T


class TransformInterpolationBuffer:
    """o3d_slam::TransformInterpolationBuffer: (time, transform) pairs pushed in order, capped at a size limit (2000,
    TransformInterpolationBuffer.cpp:16) with the oldest dropped first.  Departure: latest_measurement honours its offset
    (the reference's const overload ignores it, which is what makes its velocity estimate throw)."""

    def __init__(self, bufferSize=2000):
        if not (_is_int(bufferSize) and bufferSize >= 1):
            raise InvalidParameter(f"bufferSize must be an integer >= 1, got {bufferSize!r}")
        self.bufferSizeLimit_ = bufferSize
        self.transforms_ = []

    def push(self, time, tf) -> bool:
        """False (and nothing stored) for a time earlier than the earliest or than the latest measurement
        (TransformInterpolationBuffer.cpp:22-46)."""
        if self.transforms_ and (time < self.earliest_time() or time < self.latest_time()):
            return False
        self.transforms_.append((int(time), np.array(tf, np.float64).reshape(4, 4)))
        self._trim()
        return True

    def _trim(self):
        while len(self.transforms_) > self.bufferSizeLimit_:
            self.transforms_.pop(0)

    def setSizeLimit(self, n):
        if not (_is_int(n) and n >= 1):
            raise InvalidParameter(f"the size limit must be an integer >= 1, got {n!r}")
        self.bufferSizeLimit_ = n
        self._trim()

    def clear(self):
        self.transforms_ = []

    def empty(self) -> bool:
        return not self.transforms_

    def size(self) -> int:
        return len(self.transforms_)

    def size_limit(self) -> int:
        return self.bufferSizeLimit_

    def _need(self):
        if not self.transforms_:
            raise RuntimeError("TransformInterpolationBuffer:: Empty buffer")

    def earliest_time(self):
        self._need()
        return self.transforms_[0][0]

    def latest_time(self):
        self._need()
        return self.transforms_[-1][0]

    def latest_measurement(self, offsetFromLastElement=0):
        """The measurement `offsetFromLastElement` places before the latest one; RuntimeError for an empty buffer,
        InvalidParameter for an offset that is no integer in [0, size())."""
        self._need()
        k = offsetFromLastElement
        if not (_is_int(k) and 0 <= k < len(self.transforms_)):
            raise InvalidParameter(f"offsetFromLastElement must be an integer in [0, {len(self.transforms_)}), got {k!r}")
        return self.transforms_[-1 - k]

    def has(self, time) -> bool:
        return bool(self.transforms_) and self.earliest_time() <= time <= self.latest_time()

    def lookup(self, time) -> np.ndarray:
        """The transform at `time`: stored, or interpolated between its two neighbours (lookup, :100-142)."""
        if not self.has(time):
            raise RuntimeError(f"TransformInterpolationBuffer:: Missing transform for: {time}")
        if len(self.transforms_) == 1:
            return self.transforms_[0][1].copy()
        k = next(i for i, (t, _) in enumerate(self.transforms_) if time <= t)
        if self.transforms_[k][0] == time:
            return self.transforms_[k][1].copy()
        return interpolate(self.transforms_[k - 1], self.transforms_[k], time)[1]


def getTransform(time, buffer: TransformInterpolationBuffer) -> np.ndarray:
    """o3d_slam::getTransform (:182-192): a time outside the buffer is clamped to its ends."""
    return buffer.lookup(min(max(time, buffer.earliest_time()), buffer.latest_time()))


class ConstantVelocityMotionCompensation:
    """o3d_slam::ConstantVelocityMotionCompensation over a TransformInterpolationBuffer.  The undistortion is
    reg_undistort_scan on the device; the velocity estimate is host arithmetic, written as the reference evidently intends
    it (its own throws: see TransformInterpolationBuffer) -- a departure.  `reg`: the capi.Registration to run on; without
    one the first undistortInputPointCloud creates a handle that close() frees."""

    def __init__(self, buffer: TransformInterpolationBuffer, isSpinningClockwise_=True, scanDuration_=0.1,
                 numPosesVelocityEstimation_=3, reg: "capi.Registration | None" = None):
        if not (_is_real(scanDuration_) and math.isfinite(scanDuration_) and scanDuration_ > 0.0):
            raise InvalidParameter(f"lidar scanDuration_: must be finite and > 0, got {scanDuration_!r}")   # setParameters
        if not (_is_int(numPosesVelocityEstimation_) and numPosesVelocityEstimation_ >= 1):
            raise InvalidParameter(f"numPosesVelocityEstimation_ must be an integer >= 1, got {numPosesVelocityEstimation_!r}")
        self.buffer_ = buffer
        self.isSpinningClockwise_ = bool(isSpinningClockwise_)
        self.scanDuration_ = float(scanDuration_)
        self.numPosesVelocityEstimation_ = numPosesVelocityEstimation_
        self._reg = reg
        self._own = False   # True once undistortInputPointCloud has made a handle of its own: close() frees it

    def close(self):
        """Frees the registration handle this object created (a handle given as `reg` stays the caller's)."""
        if self._own and self._reg is not None:
            self._reg.close()
            self._reg, self._own = None, False

    def computePhase(self, x, y) -> float:
        angle = math.atan2(y, x)
        wrapped = angle + 2.0 * math.pi if angle < 0.0 else angle
        if wrapped == 0.0:
            return 0.0
        return 1.0 - wrapped / (2.0 * math.pi) if self.isSpinningClockwise_ else wrapped / (2.0 * math.pi)

    def estimateLinearAndAngularVelocity(self, timestamp):
        """(linear, angular rpy) of the sensor from the latest pose and the one numPosesVelocityEstimation_ before it;
        zero while the buffer holds no more poses than that, or already holds the timestamp."""
        offset = self.numPosesVelocityEstimation_
        if self.buffer_.size() <= offset or not (self.buffer_.latest_time() < timestamp):
            return np.zeros(3), np.zeros(3)
        t1, T1 = self.buffer_.latest_measurement()
        t0, T0 = self.buffer_.latest_measurement(offset)
        dT = np.linalg.inv(T0) @ T1
        dt = (t1 - t0) * 1e-9
        if not dt > 0.0:
            raise RuntimeError("dt should be > 0!!!!")
        q = _quat_from_R(dT[:3, :3])
        return dT[:3, 3] / (dt + 1e-6), toRPY(q / np.linalg.norm(q)) / (dt + 1e-6)

    def params(self, timestamp) -> "capi.UndistortParams":
        lin, ang = self.estimateLinearAndAngularVelocity(timestamp)
        return capi.undistort_params(self.scanDuration_, lin, ang, self.isSpinningClockwise_)

    def undistortInputPointCloud(self, xyz, timestamp) -> np.ndarray:
        """n x 3 fp64 points of the raw scan, motion-compensated on the device."""
        if self._reg is None:
            self._reg, self._own = _feature_handle(), True   # kept for the next scan; close() frees it
        try:
            return self._reg.undistort_scan(xyz, self.params(timestamp))
        except RegError as e:
            raise _translate(e) from None


# ---- LidarOdometry (Odometry.cpp) --------------------------------------------------------------------------------
@dataclass
class OdometryParameters:
    """o3d_slam::OdometryParameters (Parameters.hpp:59-86), the fields LidarOdometry reads: scanMatcher_ (regType_ and its
    IcpParameters), scanProcessing_ (ratio, voxel size, cropper) and useOdometryTopic_.  `cropper_` is a crop dict of
    capi.Registration.set_target_f64; seed_, gicpEpsilon_ and minFitness_ have no field in the reference (the selection's
    seed, Open3D's epsilon and the "todo magic" 0.1 of Odometry.cpp:56)."""
    regType_: object = "PointToPlaneIcp"
    maxNumIter_: int = 50
    maxCorrespondenceDistance_: float = 0.2
    knn_: int = 5
    maxDistanceKnn_: float = 10.0
    downSamplingRatio_: float = 1.0
    voxelSize_: float = 0.03
    cropper_: dict = field(default_factory=lambda: dict(type=capi.CROP_MAX_RADIUS, radius_min=0.0, radius_max=20.0,
                                                        min_z=-10.0, max_z=10.0))
    useOdometryTopic_: bool = True
    seed_: int = 0
    gicpEpsilon_: float = 1e-3
    minFitness_: float = 0.1


class LidarOdometry:
    """o3d_slam::LidarOdometry on the device (capi.Odometry on a handle of its own): the previous cloud never leaves HBM
    between scans; the pose buffer is the host TransformInterpolationBuffer, pushed into whenever the library says
    pose_updated.  Times are integer nanoseconds.  close() frees the handle."""

    def __init__(self, params: "OdometryParameters | None" = None):
        self.odomToRangeSensorBuffer_ = TransformInterpolationBuffer()
        self._reg = self._odom = None
        self.setParameters(params if params is not None else OdometryParameters())

    def close(self):
        if self._odom is not None:
            self._odom.close()
        if self._reg is not None:
            self._reg.close()
        self._reg = self._odom = None

    def setParameters(self, p: OdometryParameters):
        """setParameters (Odometry.cpp:104-108): a new cropper and a new operator; the previous cloud and the pose stay in
        the reference, and here the object starts afresh only before its first scan."""
        if self._odom is not None and self._odom.info().has_cloud:
            raise InvalidParameter("LidarOdometry.setParameters after the first scan is not supported: the cloud lives on "
                                   "the handle of the operator it was made for")
        self.close()
        self.params_ = p
        # cloudRegistrationFactory picks the operator, and with it the configuration of the handle
        self._operator = cloudRegistrationFactory(p.regType_, p.maxCorrespondenceDistance_, p.maxNumIter_, p.knn_,
                                                  p.maxDistanceKnn_)
        estimates = not isinstance(self._operator, RegistrationIcpPointToPoint)
        self._oparams = capi.default_odometry_params(
            crop=p.cropper_, voxel_size=p.voxelSize_, down_sampling_ratio=p.downSamplingRatio_, seed=p.seed_,
            normal_knn=p.knn_ if estimates else 0, normal_radius=p.maxDistanceKnn_, gicp_epsilon=p.gicpEpsilon_,
            min_fitness=p.minFitness_, use_odometry_topic=int(bool(p.useOdometryTopic_)))
        if capi.check_odometry_params(self._operator.params(), self._oparams) != 0:
            raise InvalidParameter("LidarOdometry: parameters refused by reg_check_odometry_params")

    def _ensure(self):
        if self._odom is None:
            try:
                self._reg = capi.Registration(self._operator.params())
                self._odom = capi.Odometry(self._reg, self._oparams)
            except RegError as e:
                raise _translate(e) from None
        return self._odom

    def addRangeScan(self, cloud, timestamp) -> bool:
        """addRangeScan (Odometry.cpp:29-84): PointCloud, DataPoints or a bare N x 3 array in the sensor frame."""
        c = _cloud64(cloud)
        try:
            res = self._ensure().add_scan(c.points_, timestamp, c.normals_)
        except RegError as e:
            raise _translate(e) from None
        self.last_result = res
        if res.pose_updated:
            self.odomToRangeSensorBuffer_.push(int(timestamp), res.cumulative_matrix())
        return bool(res.accepted)

    def getOdomToRangeSensor(self, t) -> np.ndarray:
        return getTransform(t, self.odomToRangeSensorBuffer_)

    def getPreProcessedCloud(self) -> PointCloud:
        if self._odom is None:
            return PointCloud(np.empty((0, 3), np.float64))
        c = self._odom.export_cloud()
        return PointCloud(c["xyz"], c["normals"], c["covs"])

    def getBuffer(self) -> TransformInterpolationBuffer:
        return self.odomToRangeSensorBuffer_

    def hasProcessedMeasurements(self) -> bool:
        return not self.odomToRangeSensorBuffer_.empty()

    def setInitialTransform(self, initialTransform) -> bool:
        """setInitialTransform (Odometry.cpp:110-126): False while an earlier one is still pending (the reference prints
        and skips)."""
        _check_T(initialTransform, "initialTransform")
        try:
            return self._ensure().set_initial_transform(initialTransform)
        except RegError as e:
            raise _translate(e) from None


# ---- pose-graph optimisation: Open3D's GlobalOptimization as OptimizationProblem::solve runs it (OptimizationProblem.cpp,
#      SubmapCollection.cpp:322-373).  Parity with Open3D 0.15.1 is unpinned: the contract is the text of
#      include/o3dslam_reg.h ----------------------------------------------------------------------------------------------
@dataclass
class GlobalOptimizationOption:
    """open3d::pipelines::registration::GlobalOptimizationOption with the mapper's values (Parameters.hpp:142-147)."""
    max_correspondence_distance: float = 10.0
    edge_prune_threshold: float = 0.2
    preference_loop_closure: float = 2.0
    reference_node: int = 0


@dataclass
class GlobalOptimizationConvergenceCriteria:
    """open3d::pipelines::registration::GlobalOptimizationConvergenceCriteria, Open3D's defaults."""
    max_iteration: int = 100
    min_relative_increment: float = 1e-6
    min_relative_residual_increment: float = 1e-6
    min_right_term: float = 1e-6
    min_residual: float = 1e-6
    max_iteration_lm: int = 20
    upper_scale_factor: float = 2.0 / 3.0
    lower_scale_factor: float = 1.0 / 3.0


@dataclass
class PoseGraphNode:
    pose_: np.ndarray = field(default_factory=lambda: np.eye(4))


@dataclass
class PoseGraphEdge:
    source_node_id_: int = -1
    target_node_id_: int = -1
    transformation_: np.ndarray = field(default_factory=lambda: np.eye(4))
    information_: np.ndarray = field(default_factory=lambda: np.eye(6))
    uncertain_: bool = False
    confidence_: float = 1.0


class PoseGraph:
    """open3d::pipelines::registration::PoseGraph: nodes_ and edges_."""

    def __init__(self, nodes=None, edges=None):
        self.nodes_ = list(nodes) if nodes is not None else []
        self.edges_ = list(edges) if edges is not None else []

    def copy(self) -> "PoseGraph":
        return PoseGraph([PoseGraphNode(np.array(n.pose_, np.float64)) for n in self.nodes_],
                         [PoseGraphEdge(e.source_node_id_, e.target_node_id_, np.array(e.transformation_, np.float64),
                                        np.array(e.information_, np.float64), bool(e.uncertain_), float(e.confidence_))
                          for e in self.edges_])


def _pose_graph_params(option, criteria) -> "capi.PoseGraphParams":
    o = option if option is not None else GlobalOptimizationOption()
    c = criteria if criteria is not None else GlobalOptimizationConvergenceCriteria()
    for name, v in list(vars(o).items()) + list(vars(c).items()):
        if not (_is_real(v) and math.isfinite(v)):
            raise InvalidParameter(f"{name} must be a finite number, got {v!r}")
    p = capi.default_pose_graph_params(**vars(o), **vars(c))
    if capi.check_pose_graph_params(p) != 0:
        raise InvalidParameter("GlobalOptimization: a negative distance, preference or max_iteration, max_iteration_lm < 1, or "
                               "scale factors that are not 0 < lower <= upper")
    return p


def GlobalOptimization(pose_graph: PoseGraph, method=None, criteria=None, option=None, reg: "capi.Registration | None" = None):
    """open3d::pipelines::registration::GlobalOptimization on the device, in place on pose_graph: both Levenberg-Marquardt
    passes, the prunes and the reference compensation (`method` is accepted for the signature; Levenberg-Marquardt is the
    one the mapper uses and the one built).  Returns the two passes' capi.PoseGraphResult."""
    params = _pose_graph_params(option, criteria)
    n, edges = len(pose_graph.nodes_), pose_graph.edges_
    if n == 0:
        raise InvalidParameter("GlobalOptimization: the pose graph has no nodes")
    own = reg is None
    reg = reg if reg is not None else _feature_handle()
    try:
        with capi.PoseGraph(reg, params) as g:
            g.set(np.stack([_check_T(x.pose_, "pose_") for x in pose_graph.nodes_]),
                  [e.source_node_id_ for e in edges], [e.target_node_id_ for e in edges],
                  np.stack([_check_T(e.transformation_, "transformation_") for e in edges]) if edges else np.zeros((0, 4, 4)),
                  np.stack([np.asarray(e.information_, np.float64).reshape(6, 6) for e in edges]) if edges else np.zeros((0, 6, 6)),
                  [bool(e.uncertain_) for e in edges], [float(e.confidence_) for e in edges])
            res = g.global_optimize()
            out = g.get()
    except RegError as e:
        raise _translate(e) from None
    finally:
        if own:
            reg.close()
    kept = []
    for k, c in zip(out["ids"], out["confidence"]):
        e = edges[int(k)]
        kept.append(PoseGraphEdge(e.source_node_id_, e.target_node_id_, e.transformation_, e.information_, e.uncertain_, float(c)))
    pose_graph.nodes_ = [PoseGraphNode(out["poses"][i].copy()) for i in range(n)]
    pose_graph.edges_ = kept
    return res


class OptimizationProblem:
    """o3d_slam::OptimizationProblem (OptimizationProblem.cpp): collects icp.Constraint objects as buildConstraint and
    refineLoopClosure produce them, builds the pose graph and solves it on the device.  Two oddities of the reference:
    its sort of the odometry constraints compares source with the OTHER constraint's target (line 67), which is no strict
    weak order; restated as a stable sort by source index.  getOptimizedTransformIncrements returns the optimised pose
    itself, not a difference (lines 195-198); reproduced."""

    def __init__(self, option: "GlobalOptimizationOption | None" = None, reg: "capi.Registration | None" = None):
        self.option_ = option if option is not None else GlobalOptimizationOption()
        self._reg = reg
        self.odometryConstraints_, self.loopClosureConstraints_ = [], []
        self.poseGraph_, self.poseGraphOptimized_, self.poseGraphNonOptimized_ = PoseGraph(), PoseGraph(), PoseGraph()
        self.numOdometryEdgesPrev_ = 0
        self.lastResults_ = None

    def close(self):
        self._reg = None

    def setParameters(self, option: GlobalOptimizationOption):
        self.option_ = option

    def addOdometryConstraint(self, c: Constraint):
        self.odometryConstraints_.append(c)

    def addLoopClosureConstraint(self, c: Constraint):
        self.loopClosureConstraints_.append(c)

    def insertOdometryConstraints(self, cs):
        self.odometryConstraints_.extend(cs)

    def insertLoopClosureConstraints(self, cs):
        """A constraint between a pair of submaps that already has one is dropped (lines 177-189)."""
        for c in cs:
            if not any(c.sourceSubmapIdx_ == k.sourceSubmapIdx_ and c.targetSubmapIdx_ == k.targetSubmapIdx_
                       for k in self.loopClosureConstraints_):
                self.loopClosureConstraints_.append(c)

    def clearOdometryConstraints(self):
        self.odometryConstraints_.clear()

    def clearLoopClosureConstraints(self):
        self.loopClosureConstraints_.clear()

    def getLoopClosureConstraints(self):
        return self.loopClosureConstraints_

    def updateLoopClosureConstraint(self, idx: int, c: Constraint):
        if not 0 <= idx < len(self.loopClosureConstraints_):
            raise IndexError(f"loop closure constraint {idx} of {len(self.loopClosureConstraints_)}")   # vector::at
        self.loopClosureConstraints_[idx] = c

    def buildOptimizationProblem(self, submaps=None):
        """setupOdometryEdgesAndPoseGraphNodes + setupLoopClosureEdges (lines 50-121); `submaps` is unused, as there."""
        g = self.poseGraph_
        g.edges_ = []
        self.odometryConstraints_.sort(key=lambda c: c.sourceSubmapIdx_)   # stable
        for c in self.odometryConstraints_:
            if not c.targetSubmapIdx_ > c.sourceSubmapIdx_:
                raise InvalidParameter("id_source should always be less than id_target for the odometry constraints")
            g.edges_.append(PoseGraphEdge(c.sourceSubmapIdx_, c.targetSubmapIdx_, np.array(c.sourceToTarget_, np.float64),
                                          np.array(c.informationMatrix_, np.float64), False))
        if len(self.poseGraphOptimized_.edges_) > 0:
            odometry = np.linalg.inv(self.poseGraphOptimized_.nodes_[-1].pose_)
        else:
            g.nodes_.append(PoseGraphNode(np.eye(4)))
            odometry = np.eye(4)
        for c in self.odometryConstraints_[self.numOdometryEdgesPrev_:]:
            odometry = np.asarray(c.sourceToTarget_, np.float64) @ odometry
            g.nodes_.append(PoseGraphNode(np.linalg.inv(odometry)))
        self.numOdometryEdgesPrev_ = len(self.odometryConstraints_)
        for c in self.loopClosureConstraints_:
            if not c.isInformationMatrixValid_:
                raise InvalidParameter(f"Invalid information matrix between: {c.sourceSubmapIdx_} and {c.targetSubmapIdx_}")
            if not c.sourceSubmapIdx_ > c.targetSubmapIdx_:
                raise InvalidParameter("Optimization problem, loop closure constraints: source must be greater than target")
            g.edges_.append(PoseGraphEdge(c.sourceSubmapIdx_, c.targetSubmapIdx_, np.array(c.sourceToTarget_, np.float64),
                                          np.array(c.informationMatrix_, np.float64), True))

    def solve(self):
        """OptimizationProblem::solve (lines 25-44): GlobalOptimization with the criteria's defaults and this option."""
        self.poseGraphNonOptimized_ = self.poseGraph_.copy()
        self.lastResults_ = GlobalOptimization(self.poseGraph_, None, GlobalOptimizationConvergenceCriteria(), self.option_,
                                               reg=self._reg)
        self.poseGraphOptimized_ = self.poseGraph_.copy()
        return self.lastResults_

    def getOptimizedTransformIncrements(self):
        """[(dT_, submapId_)]: dT_ is the optimised pose itself (the reference's oddity)."""
        if len(self.poseGraphOptimized_.nodes_) != len(self.poseGraph_.nodes_):
            raise InvalidParameter("Graphs are not of same size, did you run the optimization?")
        return [(np.array(n.pose_, np.float64), i) for i, n in enumerate(self.poseGraphOptimized_.nodes_)]


def _apply_submap_transform(submap, T):
    submap.transform(T)


def transformSubmaps(submaps, parentIds, increments):
    """SubmapCollection::transform (SubmapCollection.cpp:322-373): every submap named by an increment moves by it; every other
    submap moves by the increment of the first ancestor (parentIds[i] = the parent of submap i) that is in the graph.
    A submap that is its own parent and not in the graph: RuntimeError("Stuck in a loop, this should not happen").  Runs on
    Submap.transform (reg_map_cloud_transform / reg_dense_map_transform): no kernel of its own."""
    increments = list(increments)
    optimized = []
    for T, idx in increments:
        if 0 <= idx < len(submaps):
            _apply_submap_transform(submaps[idx], T)
            optimized.append(idx)
    missing = [i for i in range(len(submaps)) if i not in set(optimized)]
    for idx in missing:
        current = idx
        while increments:
            current = parentIds[current]
            if current not in missing:   # the parent is in the pose graph
                _apply_submap_transform(submaps[idx], increments[current][0])   # transformIncrements.at(currentNode)
                break
            if current == parentIds[current]:
                raise RuntimeError("Stuck in a loop, this should not happen")


# ---- the mapping thread's per-scan path: SubmapCollection and Mapper (SubmapCollection.cpp, Mapper.cpp:168-484) ----
@dataclass
class SubmapParameters:
    """o3d_slam::SubmapParameters (Parameters.hpp:103-110), the place-recognition gates the collection reads, the number of
    submaps the collection may hold and magic::voxelExpansionFactorAdjacencyBasedRevisiting."""
    radius_: float = 20.0
    minNumRangeData_: int = 5
    maxNumPoints_: int = 400000
    minSecondsBetweenFeatureComputation_: float = 5.0
    adjacencyBasedRevisitingMinFitness_: float = 0.4
    numScansOverlap_: int = 3
    loopClosureSearchRadius_: float = 20.0
    minSubmapsBetweenLoopClosures_: int = 2
    maxSubmaps_: int = 64
    voxelExpansionFactor_: float = 2.5


@dataclass
class DenseMapBuilderParameters:
    """What Submap::insertScanDenseMap reads of params_.denseMapBuilder_ and of the submap's croppers: the dense map's voxel
    size, the dense-map cropper (a crop dict; its centre as given, zero is the reference), the colour range and the carving
    parameters.  carveInMapFrame=False is the reference's oddity (icp.DenseMapBuilder)."""
    mapVoxelSize_: float = 0.03
    cropper: "dict | None" = None
    colorCropper: "ColorRangeCropper | None" = None
    carving_: "SpaceCarvingParameters | None" = None
    carveInMapFrame: bool = False

    def struct(self) -> "capi.SubmapsDenseParams":
        _check_voxel_size(self.mapVoxelSize_)
        carving = self.carving_ if self.carving_ is not None else SpaceCarvingParameters()
        carving.check(self.mapVoxelSize_)
        _check_crop(self.cropper, "cropper")
        cc = self.colorCropper if self.colorCropper is not None else ColorRangeCropper()
        return capi.default_submaps_dense_params(self.cropper, cc.rgbMin_, cc.rgbMax_, carving.params(),
                                                 carve_every_n_scans=carving.carveSpaceEveryNscans_,
                                                 carve_in_map_frame=bool(self.carveInMapFrame), voxel_size=self.mapVoxelSize_)


class SubmapCollection:
    """o3d_slam::SubmapCollection on one resident capi.Submaps: every submap's map cloud, its occupancy keys and the overlap
    buffer stay on the device; the state machine runs inside the library (reg_submaps_insert_scan).  Built from a ScanToMapIcp
    it shares that object's handle and map builder cropper, so that processForScanMatchingAndMergingDevice -> register ->
    insertScan -> setAsReference never passes a cloud through the host."""

    def __init__(self, scanToMap: "ScanToMapIcp | None" = None, *, reg: "capi.Registration | None" = None,
                 params: "SubmapParameters | None" = None, mapVoxelSize_=0.03, mapBuilderCropper=None,
                 carving: "SpaceCarvingParameters | None" = None, hasNormals=True, hasCovariances=False, isUseInitialMap_=False,
                 isCarvingEnabled_=False, denseMapBuilder: "DenseMapBuilderParameters | None" = None):
        """denseMapBuilder: every submap also keeps its dense map on the device (insertScanDenseMap, getDenseMapCopy)."""
        p = params if params is not None else SubmapParameters()
        dense = denseMapBuilder.struct() if denseMapBuilder is not None else None
        c = carving if carving is not None else SpaceCarvingParameters()
        if scanToMap is not None and mapBuilderCropper is None:
            mapBuilderCropper = scanToMap.mapBuilderCropper
        _check_crop(mapBuilderCropper, "mapBuilderCropper")
        self.params_ = p
        self._own = scanToMap is None and reg is None
        if scanToMap is not None:
            scanToMap.icp._ensure()
            reg = scanToMap.icp._reg
        self._reg = reg if reg is not None else _feature_handle()
        mp = capi.default_map_cloud_params(mapBuilderCropper if mapBuilderCropper is not None else dict(type=capi.CROP_NONE),
                                           has_normals=bool(hasNormals), has_covariances=bool(hasCovariances),
                                           carve_every_n_scans=c.carveSpaceEveryNscans_, map_voxel_size=float(mapVoxelSize_),
                                           carve_voxel_size=c.voxelSize_, carve_max_ray=c.maxRaytracingLength_,
                                           carve_truncation=c.truncationDistance_, carve_min_dot=c.minDotProductWithNormal_)
        sp = capi.default_submaps_params(
            mp, max_submaps=p.maxSubmaps_, num_scans_overlap=p.numScansOverlap_, min_num_range_data=p.minNumRangeData_,
            is_use_initial_map=bool(isUseInitialMap_), is_carving_enabled=bool(isCarvingEnabled_),
            min_submaps_between_loop_closures=p.minSubmapsBetweenLoopClosures_, max_num_points=p.maxNumPoints_, radius=p.radius_,
            revisit_min_fitness=p.adjacencyBasedRevisitingMinFitness_, voxel_expansion_factor=p.voxelExpansionFactor_,
            min_seconds_between_features=p.minSecondsBetweenFeatureComputation_,
            loop_closure_search_radius=p.loopClosureSearchRadius_)
        try:
            self.submaps = capi.Submaps(self._reg, sp)
        except RegError as e:
            raise InvalidParameter(str(e)) from None      # "Num scan overlap has to be > 0" among them
        if dense is not None:
            self.submaps.enable_dense_maps(dense)
        self.lastInsert_ = self.lastDenseInsert_ = None

    def close(self):
        self.submaps.close()
        if self._own:
            self._reg.close()

    def setMapToRangeSensor(self, T):
        self.submaps.set_map_to_sensor(_check_T(T, "T"))

    def getNumSubmaps(self) -> int:
        return int(self.submaps.info().n_submaps)

    def getActiveSubmapIdx(self) -> int:
        return int(self.submaps.info().active)

    def isActiveSubmapEmpty(self) -> bool:
        return self.submaps.submap_info(self.getActiveSubmapIdx()).n_rows == 0

    def getTotalNumPoints(self) -> int:
        return int(self.submaps.info().total_points)

    def insertScan(self, rawScan, preProcessedScan, mapToRangeSensor, timestamp) -> bool:
        """SubmapCollection::insertScan.  preProcessedScan may be a DeviceCloud (then rawScan is uploaded once)."""
        T = _check_T(mapToRangeSensor, "mapToRangeSensor")
        if T is None:
            raise InvalidParameter("mapToRangeSensor is missing")
        raw = None if rawScan is None else rawScan if isinstance(rawScan, DeviceCloud) else _cloud64(rawScan, "rawScan")
        try:
            if isinstance(preProcessedScan, DeviceCloud) or isinstance(raw, DeviceCloud):
                scan = preProcessedScan if isinstance(preProcessedScan, DeviceCloud) else Submap._to_device(
                    _cloud64(preProcessedScan, "preProcessedScan"))
                raw = raw if raw is None or isinstance(raw, DeviceCloud) else Submap._to_device(raw)
                x, nr, cv, n = Submap._device_args(scan)
                rp, rn = (raw.points_.data_ptr(), int(raw.n)) if raw is not None else (None, 0)
                self.lastInsert_ = self.submaps.insert_scan_device(rp, rn, x, n, T, int(timestamp), nr, cv)
            else:
                scan = _cloud64(preProcessedScan, "preProcessedScan")
                self.lastInsert_ = self.submaps.insert_scan(raw.points_ if raw is not None else None, scan.points_, T,
                                                            int(timestamp), scan.normals_, scan.covariances_)
        except RegError as e:
            raise _translate(e) from None
        return True

    def forceNewSubmapCreation(self):
        self.lastInsert_ = self.submaps.force_new_submap()

    def insertScanDenseMap(self, submapId, rawScan, mapToRangeSensor, isPerformCarving=True) -> bool:
        """Submap::insertScanDenseMap of submap submapId (one step of SlamWrapper::denseMapWorker): rawScan is a cloud with
        optional normals and colours in the sensor frame.  Needs denseMapBuilder= at construction."""
        T = _check_T(mapToRangeSensor, "mapToRangeSensor")
        if T is None:
            raise InvalidParameter("mapToRangeSensor is missing")
        c = _cloud64(rawScan, "rawScan")
        try:
            self.lastDenseInsert_ = self.submaps.insert_scan_dense_map(int(submapId), c.points_, T, c.normals_, c.colors_,
                                                                       bool(isPerformCarving))
        except RegError as e:
            raise _translate(e) from None
        return True

    def getDenseMapCopy(self, submapId) -> PointCloud:
        """getSubmap(submapId).getDenseMapCopy().toPointCloud(): positions, normals and colours in ascending key order."""
        try:
            d = self.submaps.export_dense_submap(int(submapId), want_keys=False, want_counts=False)
        except RegError as e:
            raise _translate(e) from None
        return PointCloud(d["xyz"], d["normals"], None, d["colors"])

    def computeFeatures(self, finishedSubmapIds, now_seconds, params: "PlaceRecognitionParameters | None" = None):
        """SubmapCollection::computeFeatures for [(id, stamp)]: per id Submap::computeFeatures on the device from the resident
        map (sparse cloud, normals, FPFH, occupancy set; reg_submaps_compute_features), then the id becomes a loop-closure
        candidate.  Returns {id: (DataPoints, Feature)} of the submaps whose gate let the computation run."""
        prm = params if params is not None else PlaceRecognitionParameters()
        fp = capi.default_submap_feature_params(normal_knn=prm.normalKnn_, feature_knn=prm.featureKnn_,
                                                feature_voxel_size=prm.featureVoxelSize_, normal_radius=prm.normalEstimationRadius_,
                                                feature_radius=prm.featureRadius_)
        out = {}
        for idx, stamp in finishedSubmapIds:
            try:
                r = self.submaps.compute_features(idx, now_seconds, fp)
            except RegError as e:
                raise _translate(e) from None
            if r is not None:
                out[idx] = (DataPoints(r["xyz"], normals=r["normals"]), Feature(np.ascontiguousarray(r["fpfh"].T)))
            self.submaps.push_loop_closure_candidate(idx, stamp)
        return out

    def popFinishedSubmapIds(self):
        return self.submaps.pop_finished()

    def popLoopClosureCandidates(self):
        return self.submaps.pop_loop_closure_candidates()

    def updateAdjacencyMatrix(self, loopClosureConstraints):
        self.submaps.add_loop_closure_edges([(c.sourceSubmapIdx_, c.targetSubmapIdx_) for c in loopClosureConstraints])

    def getLoopClosureCandidatesIdxs(self, lastFinishedSubmapIdx):
        return self.submaps.loop_closure_candidates(lastFinishedSubmapIdx)

    def getSubmapPointCloud(self, idx) -> PointCloud:
        e = self.submaps.export_submap(idx)
        return PointCloud(e["xyz"], e["normals"], e["covs"])

    def getAssembledMapPointCloud(self) -> PointCloud:
        e = self.submaps.export()
        return PointCloud(e["xyz"], e["normals"], e["covs"])

    def transform(self, increments):
        """SubmapCollection::transform of [(dT, submapId)] (OptimizationProblem.getOptimizedTransformIncrements)."""
        increments = list(increments)
        try:
            self.submaps.transform([i for _, i in increments], [T for T, _ in increments])
        except RegError as e:
            if e.status == 4:
                raise RuntimeError("Stuck in a loop, this should not happen") from None
            raise _translate(e) from None

    def setAsReference(self, crop=None) -> int:
        """cropSubmap + initReference of the active submap onto the handle.  Returns the rows of the patch; 0 for an empty
        map or an empty patch (REG_EMPTY_TARGET: initReference returns false; the previous reference is gone)."""
        _check_crop(crop, "crop")
        try:
            return self.submaps.set_target(crop)
        except RegError as e:
            if e.status == 1:
                return 0
            raise _translate(e) from None


@dataclass
class MapperParameters:
    """What Mapper::addRangeMeasurement reads of o3d_slam::MapperParameters (Parameters.hpp:71,166,178-182)."""
    isUseInitialMap_: bool = False
    isMergeScansIntoMap_: bool = True
    mapMergeDelayInSeconds_: float = 10.0
    minMovementBetweenMappingSteps_: float = 0.0
    referenceCloudSettingPeriod_: float = 1.0


_TIME_MIN = -(1 << 63)


class Mapper:
    """o3d_slam::Mapper::addRangeMeasurement (Mapper.cpp:168-484) over a ScanToMapIcp, a SubmapCollection on the same handle and
    the odometry buffer: the merge cloud stays on the device between the front end, the registration and the insertion.
    Times are integer nanoseconds.  The initial guess is capi.host_mapper_initial_guess (fp64, rigid inverses).
    Departure: the map patch is cropped (and found empty) only when the reference is re-initialised; the reference crops it
    for every scan and uses it only then.  As in the reference, the stamp of the last re-initialisation moves only with a
    non-empty patch, so after an empty one every following scan tries again."""

    def __init__(self, scanToMap: ScanToMapIcp, submaps: SubmapCollection, odomToRangeSensorBuffer: "TransformInterpolationBuffer | None" = None,
                 params: "MapperParameters | None" = None):
        self.scan2MapReg_, self.submaps_ = scanToMap, submaps
        self.params_ = params if params is not None else MapperParameters()
        self.odomToRangeSensorBuffer_ = odomToRangeSensorBuffer if odomToRangeSensorBuffer is not None else TransformInterpolationBuffer()
        self.mapToRangeSensorBuffer_, self.bestGuessBuffer_ = TransformInterpolationBuffer(), TransformInterpolationBuffer()
        self.mapToRangeSensor_, self.mapToRangeSensorPrev_ = np.eye(4), np.eye(4)
        self.mapToRangeSensorLastScanInsertion_ = np.eye(4)
        self.calibration_, self.isCalibrationSet_ = np.eye(4), False
        self.isNewValueSetMapper_ = self.isIgnoreOdometryPrediction_ = False
        self.lastMeasurementTimestamp_ = self.lastReferenceInitializationTimestamp_ = _TIME_MIN
        self.initTime_ = 0
        self.nReferenceInitializations_ = 0
        self.lastBranch_ = None          # the name of the branch the last call ended in
        self.registeredCloud_ = None     # RegisteredPointCloud of the last successful call: (submapId, rawScan, transform, time)

    def setExternalOdometryFrameToCloudFrameCalibration(self, T):
        self.calibration_, self.isCalibrationSet_ = _check_T(T, "calibration"), True

    def setMapToRangeSensor(self, T):
        self.mapToRangeSensor_ = _check_T(T, "T")

    def setMapToRangeSensorInitial(self, T):
        if self.isNewValueSetMapper_:
            return
        self.mapToRangeSensorPrev_ = self.mapToRangeSensor_ = _check_T(T, "T")
        self.isNewValueSetMapper_ = True

    def loopClosureUpdate(self, correction):
        c = _check_T(correction, "correction")
        self.mapToRangeSensor_, self.mapToRangeSensorPrev_ = c @ self.mapToRangeSensor_, c @ self.mapToRangeSensorPrev_

    def hasProcessedMeasurements(self) -> bool:
        return not self.mapToRangeSensorBuffer_.empty()

    def getMapToRangeSensor(self, timestamp) -> np.ndarray:
        return getTransform(timestamp, self.mapToRangeSensorBuffer_)

    def getRegistrationBestGuess(self, timestamp) -> np.ndarray:
        return getTransform(timestamp, self.bestGuessBuffer_)

    def getAssembledMapPointCloud(self) -> PointCloud:
        return self.submaps_.getAssembledMapPointCloud()

    def _odom(self, time):
        return getTransform(time, self.odomToRangeSensorBuffer_)

    def _end(self, name, value):
        self.lastBranch_ = name
        return value

    def addRangeMeasurement(self, rawScan, timestamp) -> bool:
        """Mapper::addRangeMeasurement; a call that returns True also records registeredCloud_, what SlamWrapper.cpp:616-622
        pushes for the dense-map worker: the submap that was active BEFORE the call, the raw scan, getMapToRangeSensor(time)
        (the pose of the last measurement where the buffer has none at that time) and the time."""
        active = self.submaps_.getActiveSubmapIdx() if hasattr(self.submaps_, "getActiveSubmapIdx") else None
        ok = self._addRangeMeasurement(rawScan, timestamp)
        if ok:
            t, b = int(timestamp), self.mapToRangeSensorBuffer_
            self.registeredCloud_ = (active, rawScan, b.lookup(t) if not b.empty() and b.has(t) else self.mapToRangeSensor_, t)
        return ok

    def _addRangeMeasurement(self, rawScan, timestamp) -> bool:
        p, timestamp = self.params_, int(timestamp)
        if not p.isUseInitialMap_ and not self.isCalibrationSet_:                 # Mapper.cpp:169-174
            return self._end("calibration_not_set", False)
        self.submaps_.setMapToRangeSensor(self.mapToRangeSensor_)
        if self.submaps_.isActiveSubmapEmpty():                                   # :179-194
            if p.isUseInitialMap_:
                self.submaps_.insertScan(rawScan, rawScan, self.mapToRangeSensor_, timestamp)
                return self._end("first_scan_initial_map", True)
            self.mapToRangeSensorPrev_ = self.mapToRangeSensor_
            merge = self.scan2MapReg_.processForScanMatchingAndMergingDevice(rawScan)
            self.submaps_.insertScan(rawScan, merge, self.mapToRangeSensor_, timestamp)
            self.mapToRangeSensorBuffer_.push(timestamp, self.mapToRangeSensor_)
            self.bestGuessBuffer_.push(timestamp, self.mapToRangeSensor_)
            return self._end("first_scan", True)
        guess = lambda now: capi.host_mapper_initial_guess(self.mapToRangeSensorPrev_, self._odom(self.lastMeasurementTimestamp_),
                                                           self._odom(now), self.calibration_)
        if timestamp <= self.lastMeasurementTimestamp_:                           # :196-235: propagate by the latest odometry
            latest = self.odomToRangeSensorBuffer_.latest_time()
            self.mapToRangeSensor_ = guess(latest)
            self.mapToRangeSensorBuffer_.push(latest, self.mapToRangeSensor_)
            self.bestGuessBuffer_.push(latest, self.mapToRangeSensorPrev_)
            self.submaps_.setMapToRangeSensor(self.mapToRangeSensor_)
            self.mapToRangeSensorPrev_ = self.mapToRangeSensor_
            return self._end("out_of_order", True)
        isOdomOkay = self.odomToRangeSensorBuffer_.has(timestamp)                 # :237-241
        estimate = self.mapToRangeSensorPrev_
        if isOdomOkay and not self.isNewValueSetMapper_ and not self.isIgnoreOdometryPrediction_:   # :248-260
            estimate = guess(timestamp)
        self.isIgnoreOdometryPrediction_ = False
        merge = self.scan2MapReg_.processForScanMatchingAndMergingDevice(rawScan)   # match_ is the reading on the handle
        d = timestamp - self.lastReferenceInitializationTimestamp_                # :325-326: whole milliseconds, truncated
        passed = (d // 1_000_000 if d >= 0 else -((-d) // 1_000_000)) / 1e3
        if self.isNewValueSetMapper_ or passed >= p.referenceCloudSettingPeriod_:  # :329-347
            cropper = self.scan2MapReg_.scanMatcherCropper
            crop = None if cropper is None else dict(cropper, center=tuple(float(v) for v in self.mapToRangeSensor_[:3, 3]))
            if self.submaps_.setAsReference(crop) == 0:                           # any other error is raised, not swallowed
                return self._end("empty_map_patch", False)                        # :310-316, :343-346
            self.lastReferenceInitializationTimestamp_ = timestamp                # :341: only with a non-empty patch
            self.nReferenceInitializations_ += 1
        corrected, branch = np.asarray(estimate, np.float32), "registered"
        try:
            corrected = self.scan2MapReg_.register(corrected)[0]                  # :372-373
        except RuntimeError:
            branch = "icp_exception"                                              # :400-402: the initial guess stays
        if self.isNewValueSetMapper_:                                             # :420-435
            self.initTime_ = timestamp
            self.mapToRangeSensorPrev_ = self.mapToRangeSensor_
            self.mapToRangeSensorBuffer_.push(timestamp, self.mapToRangeSensor_)
            self.bestGuessBuffer_.push(timestamp, estimate)
            self.isNewValueSetMapper_, self.isIgnoreOdometryPrediction_ = False, True
            return self._end("new_value_set", True)
        self.mapToRangeSensor_ = np.asarray(corrected, np.float64)                # :438-442
        self.mapToRangeSensorBuffer_.push(timestamp, self.mapToRangeSensor_)
        self.bestGuessBuffer_.push(timestamp, estimate)
        self.submaps_.setMapToRangeSensor(self.mapToRangeSensor_)
        sinceInit = (timestamp - self.initTime_) * 1e-9
        if p.isUseInitialMap_ and (not p.isMergeScansIntoMap_ or sinceInit < p.mapMergeDelayInSeconds_):   # :445-459
            self.lastMeasurementTimestamp_, self.mapToRangeSensorPrev_ = timestamp, self.mapToRangeSensor_
            return self._end("merge_delay", True)
        L, M = self.mapToRangeSensorLastScanInsertion_, self.mapToRangeSensor_    # :463-469: |R_L^T (t_M - t_L)|
        d = M[:3, 3] - L[:3, 3]
        m = [(L[0, i] * d[0] + L[1, i] * d[1]) + L[2, i] * d[2] for i in range(3)]
        if not math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) < p.minMovementBetweenMappingSteps_:
            self.submaps_.insertScan(rawScan, merge, self.mapToRangeSensor_, timestamp)
            self.mapToRangeSensorLastScanInsertion_ = self.mapToRangeSensor_
        else:
            branch += "_moved_too_little"
        self.lastMeasurementTimestamp_, self.mapToRangeSensorPrev_ = timestamp, self.mapToRangeSensor_
        return self._end(branch, True)


# ---- pose-graph constraints from the resident collection (constraint_builders.cpp, PlaceRecognition.cpp:50-176,
#      SlamWrapper.cpp:1018-1090) --------------------------------------------------------------------------------
@dataclass
class PlaceRecognitionConsistencyCheckParameters:
    """o3d_slam::PlaceRecognitionConsistencyCheckParameters (Parameters.hpp:112-119): radians and metres."""
    maxDriftRoll_: float = math.pi / 2
    maxDriftPitch_: float = math.pi / 2
    maxDriftYaw_: float = math.pi / 2
    maxDriftX_: float = 10.0
    maxDriftY_: float = 10.0
    maxDriftZ_: float = 15.0


@dataclass
class LoopClosureParameters:
    """What buildLoopClosureConstraints reads: placeRecognition_ (the RANSAC fields, Parameters.hpp:127-135), its consistency
    check, the refinement operator (cloudRegistration: one of the RegistrationIcp* classes, its maxCorrespondenceDistance_ and
    max_iteration_), the map voxel size behind the overlap voxel, and the sampler's seed."""
    placeRecognition_: PlaceRecognitionParameters = field(default_factory=PlaceRecognitionParameters)
    consistencyCheck_: PlaceRecognitionConsistencyCheckParameters = field(default_factory=PlaceRecognitionConsistencyCheckParameters)
    maxIcpCorrespondenceDistance_: float = 0.3
    minRefinementFitness_: float = 0.7
    cloudRegistration: object = None
    mapVoxelSize_: float = 0.03
    seed: int = 0

    def struct(self) -> "capi.LoopClosureParams":
        op = self.cloudRegistration if self.cloudRegistration is not None else RegistrationIcpPointToPlane(
            self.maxIcpCorrespondenceDistance_, 30)
        voxel = 0.04 if abs(self.mapVoxelSize_) <= 1e-3 else self.mapVoxelSize_          # getMapVoxelSize
        refine = capi.constraint_params(op.params().cost, op.max_iteration_, True, False, True, 20.0 * voxel,
                                        op.maxCorrespondenceDistance_, self.maxIcpCorrespondenceDistance_)
        pr, cc = self.placeRecognition_, self.consistencyCheck_
        return capi.loop_closure_params(refine, pr.ransacMaxCorrespondenceDistance_, pr.ransacModelSize_, pr.ransacNumIter_,
                                        pr.ransacProbability_, pr.correspondenceCheckerDistance_, pr.correspondenceCheckerEdgeLength_,
                                        self.seed, pr.ransacMinCorrespondenceSetSize_, self.minRefinementFitness_,
                                        (cc.maxDriftRoll_, cc.maxDriftPitch_, cc.maxDriftYaw_, cc.maxDriftX_, cc.maxDriftY_, cc.maxDriftZ_))


def isRegistrationConsistent(T, consistencyCheck: "PlaceRecognitionConsistencyCheckParameters | None" = None) -> bool:
    """PlaceRecognition::isRegistrationConsistent (reg_host_registration_consistent)."""
    c = consistencyCheck if consistencyCheck is not None else PlaceRecognitionConsistencyCheckParameters()
    return capi.host_registration_consistent(_check_T(T, "T"), (c.maxDriftRoll_, c.maxDriftPitch_, c.maxDriftYaw_, c.maxDriftX_,
                                                                c.maxDriftY_, c.maxDriftZ_))[0]


def _constraint_of(r: "capi.ConstraintResult", isOdometry: bool) -> Constraint:
    return Constraint(int(r.source), int(r.target), r.T_matrix(), r.information_matrix(), bool(r.information_estimated), isOdometry)


def _collection_call(fn, *args):
    try:
        return fn(*args)
    except RegError as e:
        raise _translate(e) from None


def _sc_buildOdometryConstraint(self, sourceIdx, targetIdx, isRefineOdometryConstraintsBetweenSubmaps_=False) -> Constraint:
    """o3d_slam::buildOdometryConstraint (constraint_builders.cpp:33-41) between two resident submaps."""
    p = self.submaps.default_odometry_constraint_params(isRefineOdometryConstraintsBetweenSubmaps_)
    return _constraint_of(_collection_call(self.submaps.build_constraint, sourceIdx, targetIdx, p), True)


def _sc_computeOdometryConstraints(self, finishedSubmapIds=None, isRefineOdometryConstraintsBetweenSubmaps_=False) -> int:
    """SubmapCollection::computeOdometryConstraints into the list the collection owns: of [(id, stamp)] (or ids), or -- with
    None -- the overload without candidates.  Returns how many were added."""
    ids = None if finishedSubmapIds is None else [i[0] if isinstance(i, (tuple, list)) else i for i in finishedSubmapIds]
    p = self.submaps.default_odometry_constraint_params(isRefineOdometryConstraintsBetweenSubmaps_)
    return _collection_call(self.submaps.compute_odometry_constraints, ids, p)


def _sc_getOdometryConstraints(self) -> list:
    return [Constraint(c["source"], c["target"], c["T"], c["information"], c["information_valid"], c["is_odometry"])
            for c in self.submaps.odometry_constraints()]


def _sc_buildLoopClosureConstraints(self, loopClosureCandidatesIdxs, params: "LoopClosureParameters | None" = None,
                                    withVerdicts=False):
    """SubmapCollection::buildLoopClosureConstraints (SubmapCollection.cpp:291-305) of [(id, stamp)]: per entry
    PlaceRecognition::buildLoopClosureConstraints on the stored features and the resident maps.  Returns the accepted
    Constraints, each with `timestamp_`; with `withVerdicts` also every capi.LoopClosureVerdict."""
    p = (params if params is not None else LoopClosureParameters()).struct()
    out, verdicts = [], []
    for idx, stamp in loopClosureCandidatesIdxs:
        for v in _collection_call(self.submaps.build_loop_closure_constraints, idx, stamp, p):
            verdicts.append(v)
            if v.verdict == capi.LC_ACCEPTED:
                c = _constraint_of(v.constraint, False)
                c.timestamp_ = int(v.stamp_ns)
                out.append(c)
    return (out, verdicts) if withVerdicts else out


def _sc_computeFeatures(self, finishedSubmapIds, now_seconds, params: "PlaceRecognitionParameters | None" = None,
                        computeOdometryConstraints=False):
    """As before; with computeOdometryConstraints it ends, as the reference does (SubmapCollection.cpp:276), in
    computeOdometryConstraints(finishedSubmapIds)."""
    finishedSubmapIds = list(finishedSubmapIds)
    out = _sc_computeFeatures_before(self, finishedSubmapIds, now_seconds, params)
    if computeOdometryConstraints:
        self.computeOdometryConstraints(finishedSubmapIds)
    return out


_sc_computeFeatures_before = SubmapCollection.computeFeatures
SubmapCollection.computeFeatures = _sc_computeFeatures
SubmapCollection.buildOdometryConstraint = _sc_buildOdometryConstraint
SubmapCollection.computeOdometryConstraints = _sc_computeOdometryConstraints
SubmapCollection.getOdometryConstraints = _sc_getOdometryConstraints
SubmapCollection.buildLoopClosureConstraints = _sc_buildLoopClosureConstraints


def closeLoops(collection: SubmapCollection, problem: OptimizationProblem, mapper, candidates, params=None):
    """One pass of SlamWrapper::loopClosureWorker and updateSubmapsAndTrajectory (SlamWrapper.cpp:1018-1090) without threads:
    the loop-closure constraints of `candidates` [(id, stamp)]; none accepted: returns []; else the collection's odometry
    constraints plus the missing ones (built on a copy of the list, as there), the optimisation problem rebuilt and solved,
    the submaps transformed, the mapper's pose corrected by the increment of the latest constraint's source, the loop-closure
    constraints reset to the identity and the adjacency matrix updated.  `mapper` may be None.  Returns the accepted constraints."""
    loopClosureConstraints = collection.buildLoopClosureConstraints(candidates, params)
    if not loopClosureConstraints:
        return []
    odometryConstraints = collection.getOdometryConstraints()
    have = [(c.sourceSubmapIdx_, c.targetSubmapIdx_) for c in odometryConstraints]
    for a, b in collection.submaps.odometry_constraint_pairs(None, have):
        odometryConstraints.append(collection.buildOdometryConstraint(a, b))
    problem.clearOdometryConstraints()
    problem.insertLoopClosureConstraints(loopClosureConstraints)
    problem.insertOdometryConstraints(odometryConstraints)
    problem.buildOptimizationProblem(collection)
    problem.solve()
    increments = problem.getOptimizedTransformIncrements()
    collection.transform(increments)
    latest = max(loopClosureConstraints, key=lambda c: c.timestamp_)
    if not latest.sourceSubmapIdx_ > latest.targetSubmapIdx_:
        raise InvalidParameter("update submaps and trajectory: the source of a loop closure must be greater than its target")
    if mapper is not None:
        mapper.loopClosureUpdate(increments[latest.sourceSubmapIdx_][0])
    reset = []
    for i, old in enumerate(problem.getLoopClosureConstraints()):
        c = Constraint(old.sourceSubmapIdx_, old.targetSubmapIdx_, np.eye(4), old.informationMatrix_, old.isInformationMatrixValid_,
                       old.isOdometryConstraint_)
        c.timestamp_ = getattr(old, "timestamp_", 0)
        problem.updateLoopClosureConstraint(i, c)
        reset.append(c)
    collection.updateAdjacencyMatrix(reset)
    return loopClosureConstraints
