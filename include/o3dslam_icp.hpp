// o3dslam_icp.hpp -- header-only C++ host-side mirror of the reference's registration object for the hot
// path, over the C ABI (o3dslam_reg.h).  Same method names, argument meaning and error behaviour as
//   PointMatcher<float>::ICP          libpointmatcher/pointmatcher/PointMatcher.h:1023-1060, ICP.cpp:793-898
// as used by o3d_slam::Mapper (open3d_slam/src/Mapper.cpp:343,372-373).  No Eigen dependency: clouds are
// passed as views on the caller's memory, which for a PointMatcher<float>::DataPoints is
//   DataPointsView{ dp.features.data(), dp.features.rows() /*4*/, dp.getNbPoints(),
//                   dp.getDescriptorViewByName("normals").data(), 3 }      (column-major Eigen == AoS per point)
// and transforms as column-major float[16] == Eigen::Matrix4f::data().
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "o3dslam_reg.h"

namespace o3dreg {

// exception names follow the reference (PointMatcher.h:130-160, DataPoints.h)
struct ConvergenceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct InvalidField : std::runtime_error { using std::runtime_error::runtime_error; };
struct InvalidParameter : std::runtime_error { using std::runtime_error::runtime_error; };
struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };

struct DataPointsView {
    const float* features = nullptr;   // {x,y,z,1} per point (stride 4) or packed xyz (stride 3)
    int64_t feature_stride = 4;
    int64_t n = 0;
    const float* normals = nullptr;    // descriptor "normals", 3 per point
    int64_t normal_stride = 3;
    const float* covariances = nullptr;  // GICP only, 6 per point
    bool on_device = false;            // pointers are HIP device pointers (already resident in HBM)
    int64_t getNbPoints() const { return n; }
};

using TransformationParameters = std::array<float, 16>;  // column-major 4x4

inline TransformationParameters identity4() {
    TransformationParameters T{};
    T[0] = T[5] = T[10] = T[15] = 1.f;
    return T;
}

class ICP {
public:
    ICP() { reg_default_params(&params_); }
    ~ICP() { if (h_) reg_destroy(h_); }
    ICP(const ICP&) = delete;
    ICP& operator=(const ICP&) = delete;

    // ICPChainBase::setDefault (ICP.cpp:100-113); drops a chain set by setPmChain (the default chain is knn 1, no robust filter)
    void setDefault() { reg_default_params(&params_); has_chain_ = false; has_ternary_ = false; reset(); }
    // the chain of open3d_slam_ros/param/icp.yaml (what Mapper loads through loadFromYaml); drops a setPmChain chain
    void setShippedChain() { reg_shipped_params(&params_); has_chain_ = false; has_ternary_ = false; reset(); }
    // direct access to the string-free parameter block (call before the first initReference)
    reg_params& parameters() { reset(); return params_; }
    // libpointmatcher chain extension (reg_set_pm_chain: k-NN matching, RobustOutlierFilter, PointToPoint, and the
    // MinDist / MedianDist / VarTrimmedDist outlier filters: use_min_dist_filter, use_median_dist, use_var_trimmed and
    // their parameters; start from reg_default_pm_chain).  The chain is kept and re-applied whenever parameters()
    // re-creates the handle (the robust state then starts afresh, as with a new filter); setting it resets the robust
    // state.
    void setPmChain(const reg_pm_chain& c) {
        chain_ = c;
        has_chain_ = true;
        if (h_) check(reg_set_pm_chain(h_, &chain_));
        else ensure();
    }

    // degeneracyAwareness EqualityConstraints (X-ICP, ternary; reg_set_ternary_xicp): start from
    // reg_default_ternary_xicp, set enabled = 1.  Kept and re-applied like the chain; not together with
    // parameters().use_xicp or a SolutionRemapping chain (InvalidParameter).
    void setTernaryXicp(const reg_ternary_xicp& t) {
        ternary_ = t;
        ternary_.struct_size = (int32_t)sizeof(reg_ternary_xicp);
        has_ternary_ = true;
        if (h_) check(reg_set_ternary_xicp(h_, &ternary_));
        else ensure();
    }
    // its analysis of the last iteration of the last compute()
    reg_ternary_xicp_result localizability() {
        ensure();
        reg_ternary_xicp_result r{};
        r.struct_size = (int32_t)sizeof(reg_ternary_xicp_result);
        check(reg_get_ternary_xicp(h_, &r));
        return r;
    }

    // VarTrimmedDistOutlierFilter's "Optimized ratio" of the last iteration, the rank it came from and n = N knn
    struct VarTrim { float ratio; int64_t index; int64_t n_total; };
    VarTrim varTrim() {
        ensure();
        VarTrim v{};
        check(reg_get_var_trim(h_, &v.ratio, &v.index, &v.n_total));
        return v;
    }

    bool hasMap() const { return matcherIsInitialized_; }
    bool getMaxNumIterationsReached() const { return last_.max_iter_reached != 0; }
    const reg_result& lastResult() const { return last_; }

    // ICP::initReference (ICP.cpp:847-898): false on an empty reference.
    bool initReference(const DataPointsView& referenceIn) {
        ensure();
        if (referenceIn.getNbPoints() == 0) { matcherIsInitialized_ = false; return false; }
        check(reg_set_target(h_, referenceIn.features, referenceIn.feature_stride, referenceIn.normals,
                             referenceIn.normal_stride, referenceIn.covariances, referenceIn.n,
                             referenceIn.on_device ? 1 : 0));
        matcherIsInitialized_ = true;
        return true;
    }

    // ICP::compute (ICP.cpp:813-844)
    TransformationParameters compute(const DataPointsView& readingIn, const DataPointsView& referenceIn,
                                     const TransformationParameters& T_refIn_readIn,
                                     bool initializeMatcherWithInputReference = true) {
        ensure();
        if (initializeMatcherWithInputReference || !matcherIsInitialized_)
            if (!initReference(referenceIn)) return identity4();
        if (readingIn.getNbPoints() == 0) throw std::runtime_error("The reading point cloud is empty.");
        TransformationParameters out = T_refIn_readIn;
        check(reg_compute(h_, readingIn.features, readingIn.feature_stride, readingIn.normals,
                          readingIn.normal_stride, readingIn.covariances, readingIn.n, readingIn.on_device ? 1 : 0,
                          T_refIn_readIn.data(), out.data(), &last_));
        return out;
    }
    TransformationParameters operator()(const DataPointsView& readingIn, const DataPointsView& referenceIn) {
        return compute(readingIn, referenceIn, identity4(), true);
    }

    // The scan as Mapper::addRangeMeasurement holds it before open3dToPointmatcher (Mapper.cpp:288-289): Open3D's fp64
    // arrays (points_ / normals_ n x 3 doubles).  Cast on the device (open3d_conversions.cpp:57-118), then compute().
    TransformationParameters computeF64(const double* points, const double* normals, int64_t n, bool on_device,
                                        const TransformationParameters& T_refIn_readIn) {
        ensure();
        if (!matcherIsInitialized_) throw std::runtime_error("You must call initReference first");
        if (n == 0) throw std::runtime_error("The reading point cloud is empty.");
        check(reg_set_source_f64(h_, points, normals, nullptr, n, on_device ? 1 : 0));
        TransformationParameters out = T_refIn_readIn;
        check(reg_register(h_, T_refIn_readIn.data(), out.data(), &last_));
        return out;
    }

    // ---- submap-pair constraints (constraint_builders.cpp:43-90, PlaceRecognition.cpp:97-149) -----------------------------
    // The front of buildConstraint in one call (reg_set_pair_overlap_f64): computeIndicesOfOverlappingPoints at
    // sourceToTarget (column-major double[16] == Eigen::Matrix4d::data(), nullptr: identity), SelectByIndex + fp32 cast on
    // the device, the selected target as the reference and the selected source as the reading.  Open3D's fp64 arrays:
    // points / normals n x 3, covariances n x 9 doubles (nullptr where the cost does not need them).  Then registerPair()
    // and informationMatrix(); an empty overlap throws std::runtime_error (REG_EMPTY_TARGET).
    struct PairOverlap { int64_t n_source; int64_t n_target; };
    PairOverlap setPairOverlap(const double* srcPoints, const double* srcNormals, const double* srcCovs, int64_t n,
                               const double* tgtPoints, const double* tgtNormals, const double* tgtCovs, int64_t m,
                               bool on_device, const double* sourceToTarget, double voxelSize,
                               int32_t minNumPointsPerVoxel = 1) {
        ensure();
        matcherIsInitialized_ = false;
        pair_ = PairOverlap{0, 0};
        check(reg_set_pair_overlap_f64(h_, srcPoints, srcNormals, srcCovs, n, tgtPoints, tgtNormals, tgtCovs, m,
                                       on_device ? 1 : 0, sourceToTarget, voxelSize, minNumPointsPerVoxel, &pair_.n_source,
                                       &pair_.n_target));
        matcherIsInitialized_ = true;
        return pair_;
    }
    // registration of the pair set by setPairOverlap, from T_init
    TransformationParameters registerPair(const TransformationParameters& T_init) {
        ensure();
        TransformationParameters out = T_init;
        check(reg_register(h_, T_init.data(), out.data(), &last_));
        return out;
    }
    // GetInformationMatrixFromPointClouds on the clouds currently set (row-major 6 x 6, rotation first); *nPairs: the
    // number of correspondences within the distance that the sum ran over
    std::array<double, 36> informationMatrix(const TransformationParameters& T, float maxCorrespondenceDistance,
                                             int64_t* nPairs = nullptr) {
        ensure();
        std::array<double, 36> info{};
        int64_t n_pairs = 0;
        check(reg_information_matrix(h_, T.data(), maxCorrespondenceDistance, info.data(), &n_pairs));
        if (nPairs) *nPairs = n_pairs;
        return info;
    }
    // positions of the selected points in the clouds given to setPairOverlap (SelectByIndex's index lists, ascending)
    std::vector<int32_t> pairSourceIndices() {
        ensure();
        std::vector<int32_t> idx((size_t)pair_.n_source);
        if (!idx.empty()) check(reg_get_source_source_indices(h_, idx.data()));
        return idx;
    }
    std::vector<int32_t> pairTargetIndices() {
        ensure();
        std::vector<int32_t> idx((size_t)pair_.n_target);
        if (!idx.empty()) check(reg_get_target_source_indices(h_, idx.data()));
        return idx;
    }

    // ---- the scan front end (ScanToMapRegistration.cpp:36-69) ---------------------------------------------
    // ScanToMapIcp::processForScanMatchingAndMerging in one call (reg_process_scan): wide crop, VoxelDownSample, normals
    // where the cloud brings none, RandomDownSample, the merge cloud into the caller's fp64 arrays (n rows each; normals /
    // covariances may be nullptr), narrow crop + fp32 cast installed as the reading.  Then registerPair(T_init) -- the
    // reference is the one given to initReference -- and scanMatchIndices().  Empty after a crop: std::runtime_error.
    reg_scan_result processScan(const double* points, const double* normals, const double* covs, int64_t n, bool on_device,
                                const reg_scan_params& scanParams, double* mergePoints, double* mergeNormals = nullptr,
                                double* mergeCovs = nullptr) {
        ensure();
        reg_scan_params p = scanParams;
        p.struct_size = (int32_t)sizeof(reg_scan_params);
        scan_ = reg_scan_result{};
        scan_.struct_size = (int32_t)sizeof(reg_scan_result);
        check(reg_process_scan(h_, points, normals, covs, n, on_device ? 1 : 0, &p, mergePoints, mergeNormals, mergeCovs, &scan_));
        return scan_;
    }
    // rows of the merge cloud that form the reading (match_), ascending
    std::vector<int32_t> scanMatchIndices() {
        ensure();
        std::vector<int32_t> idx((size_t)scan_.n_match);
        if (!idx.empty()) check(reg_get_source_source_indices(h_, idx.data()));
        return idx;
    }

    // ---- one process per GPU, reading partitioned over the group (BASELINE config C4) --------------------------------
    // Rank 0 creates the 128-byte id (ICP::makeGroupId) and hands it to the other ranks; every rank joins with its rank.
    static std::array<char, REG_DIST_ID_BYTES> makeGroupId() {
        std::array<char, REG_DIST_ID_BYTES> id{};
        if (reg_dist_get_unique_id(id.data()) != REG_OK) throw DeviceError("ncclGetUniqueId failed (is librccl loadable?)");
        return id;
    }
    void joinGroup(const std::array<char, REG_DIST_ID_BYTES>& id, int rank, int n_ranks) {
        ensure();
        check(reg_dist_init(h_, id.data(), rank, n_ranks));
    }
    void leaveGroup() { if (h_) check(reg_dist_shutdown(h_)); }
    // ICP::compute for THIS RANK'S SLICE of the reading; collective: every rank calls it with the same T and returns the
    // same transform (lastResult() carries the global figures).  The reference is the one given to initReference on
    // every rank (replicated).
    TransformationParameters computePartitioned(const DataPointsView& readingSlice,
                                                const TransformationParameters& T_refIn_readIn) {
        ensure();
        if (!matcherIsInitialized_) throw std::runtime_error("You must call initReference first");
        if (readingSlice.getNbPoints() == 0) throw std::runtime_error("The reading point cloud is empty.");
        check(reg_set_source(h_, readingSlice.features, readingSlice.feature_stride, readingSlice.normals,
                             readingSlice.normal_stride, readingSlice.covariances, readingSlice.n,
                             readingSlice.on_device ? 1 : 0));
        TransformationParameters out = T_refIn_readIn;
        check(reg_dist_register(h_, T_refIn_readIn.data(), out.data(), &last_));
        return out;
    }

private:
    void reset() { if (h_) { reg_destroy(h_); h_ = nullptr; } matcherIsInitialized_ = false; }
    void ensure() {
        if (h_) return;
        params_.struct_size = (int32_t)sizeof(reg_params);
        reg_status s = reg_create(&params_, &h_);
        if (s != REG_OK) {
            std::string msg = h_ ? reg_last_error(h_) : "reg_create rejected the parameters";
            if (h_) { reg_destroy(h_); h_ = nullptr; }
            if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
            throw InvalidParameter(msg);
        }
        if (has_chain_) {
            const reg_status cs = reg_set_pm_chain(h_, &chain_);
            if (cs != REG_OK) {
                const std::string msg = reg_last_error(h_);
                reg_destroy(h_);
                h_ = nullptr;
                if (cs == REG_DEVICE_ERROR) throw DeviceError(msg);
                throw InvalidParameter("reg_set_pm_chain: the chain does not fit the parameters (" + std::to_string((int)cs) + ") " + msg);
            }
        }
        if (has_ternary_) {
            const reg_status ts = reg_set_ternary_xicp(h_, &ternary_);
            if (ts != REG_OK) {
                const std::string msg = reg_last_error(h_);
                reg_destroy(h_);
                h_ = nullptr;
                if (ts == REG_DEVICE_ERROR) throw DeviceError(msg);
                throw InvalidParameter("reg_set_ternary_xicp: (" + std::to_string((int)ts) + ") " + msg);
            }
        }
    }
    void check(reg_status s) {
        if (s == REG_OK) return;
        const std::string msg = reg_last_error(h_);
        switch (s) {
            case REG_NO_CORRESPONDENCES: throw ConvergenceError(msg);
            case REG_MISSING_FIELD: throw InvalidField(msg);
            case REG_BAD_ARGUMENT: throw InvalidParameter(msg);
            case REG_DEVICE_ERROR: throw DeviceError(msg);
            default: throw std::runtime_error(msg);
        }
    }
    reg_params params_;
    reg_pm_chain chain_{};
    bool has_chain_ = false;
    reg_ternary_xicp ternary_{};
    bool has_ternary_ = false;
    reg_handle* h_ = nullptr;
    reg_result last_{};
    PairOverlap pair_{0, 0};
    reg_scan_result scan_{};
    bool matcherIsInitialized_ = false;
};

// o3d_slam::computeIndicesOfOverlappingPoints (helpers.cpp:320-345) on the device (reg_overlap_indices): the ascending
// indices of the points of either fp64 cloud (n x 3 / m x 3 doubles, host memory) whose voxel holds at least
// minNumPointsPerVoxel points of the target and of the source moved by sourceToTarget (column-major double[16], nullptr:
// identity).  The reference emits the lists in std::unordered_map order.
struct OverlapIndices { std::vector<int32_t> source, target; };
inline OverlapIndices overlapIndices(const double* source, int64_t n, const double* target, int64_t m,
                                     const double* sourceToTarget, double voxelSize, int32_t minNumPointsPerVoxel = 1,
                                     int device = 0) {
    reg_params p;
    reg_default_params(&p);
    p.cost = REG_COST_O3D_P2P;   // no field requirements: the handle only lends its stream and workspace
    p.device = device;
    reg_handle* h = nullptr;
    reg_status s = reg_create(&p, &h);
    OverlapIndices out;
    std::string msg;
    if (s == REG_OK) {
        out.source.resize((size_t)(n > 0 ? n : 0));
        out.target.resize((size_t)(m > 0 ? m : 0));
        int64_t ns = 0, nt = 0;
        s = reg_overlap_indices(h, source, n, target, m, 0, sourceToTarget, voxelSize, minNumPointsPerVoxel, out.source.data(),
                                &ns, out.target.data(), &nt);
        out.source.resize((size_t)ns);
        out.target.resize((size_t)nt);
    }
    if (s != REG_OK) msg = h ? reg_last_error(h) : "reg_create rejected the parameters";
    if (h) reg_destroy(h);
    if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
    if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
    if (s != REG_OK) throw std::runtime_error(msg);
    return out;
}

// The front of place recognition on the device (contract in o3dslam_reg.h; PARITY UNPINNED against Open3D
// 0.15.1).  Both run on a handle of their own, which only lends its stream and workspace.
template <class F>
inline void withFeatureHandle(int device, F&& call) {
    reg_params p;
    reg_default_params(&p);
    p.cost = REG_COST_O3D_P2P;
    p.device = device;
    reg_handle* h = nullptr;
    reg_status s = reg_create(&p, &h);
    if (s == REG_OK) s = call(h);
    const std::string msg = s == REG_OK ? "" : (h ? reg_last_error(h) : "reg_create rejected the parameters");
    if (h) reg_destroy(h);
    if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
    if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
    if (s != REG_OK) throw std::runtime_error(msg);
}

// ComputeFPFHFeature(cloud, KDTreeSearchParamHybrid(radius, maxNn)) (Submap.cpp:267-269): points / normals n x 3 floats in
// host memory; returns n x 33 doubles, row i = column i of Open3D's Feature::data_.
inline std::vector<double> computeFPFH(const float* points, const float* normals, int64_t n, float radius, int maxNn = 100,
                                       int device = 0) {
    std::vector<double> fpfh((size_t)(n > 0 ? n : 0) * 33);
    withFeatureHandle(device, [&](reg_handle* h) {
        return reg_compute_fpfh(h, points, 3, normals, 3, n, 0, maxNn, radius, fpfh.data(), nullptr, nullptr, nullptr);
    });
    return fpfh;
}

// The correspondence set RegistrationRANSACBasedOnFeatureMatching(..., mutual_filter, ...) forms before it samples
// (PlaceRecognition.cpp:81-84): rows of `source` (na x dim) and `target` (nb x dim) doubles in host memory; interleaved
// (source, target) index pairs -- the mutual nearest neighbours when there are at least ransacN of them, else every
// (a, nearest b), as Open3D falls back.
inline std::vector<int32_t> matchFeatures(const double* source, int64_t na, const double* target, int64_t nb, int dim = 33,
                                          bool mutualFilter = true, int ransacN = 3, int device = 0) {
    std::vector<int32_t> nn((size_t)(na > 0 ? na : 0)), mutual(mutualFilter ? 2 * nn.size() : 0);
    int64_t k = 0;
    withFeatureHandle(device, [&](reg_handle* h) {
        return reg_match_features(h, source, na, target, nb, dim, 0, nn.data(), nullptr, mutualFilter ? mutual.data() : nullptr, &k);
    });
    if (mutualFilter && k >= ransacN) {
        mutual.resize((size_t)(2 * k));
        return mutual;
    }
    std::vector<int32_t> all(2 * nn.size());
    for (size_t a = 0; a < nn.size(); ++a) {
        all[2 * a] = (int32_t)a;
        all[2 * a + 1] = nn[a];
    }
    return all;
}

// PointCloud::VoxelDownSample / RandomDownSample on the device (contract in o3dslam_reg.h; PARITY UNPINNED
// against Open3D 0.15.1): Open3D's fp64 arrays in host memory (points / normals n x 3, covs n x 9 doubles; normals and covs
// may be nullptr).  voxelDownSample: the grid starts at min_bound - voxelSize / 2, averaged normals are not re-normalised,
// voxels in ascending (z, y, x) index.  randomDownSample: the kept set is a function of (n, ratio, seed) only; `indices`
// are the ascending kept rows.
struct SampledCloud {
    std::vector<double> points, normals, covs;
    std::vector<int32_t> indices;   // randomDownSample only
    int64_t size() const { return (int64_t)(points.size() / 3); }
};
inline SampledCloud voxelDownSample(const double* points, const double* normals, const double* covs, int64_t n,
                                    double voxelSize, int device = 0) {
    const size_t rows = (size_t)(n > 0 ? n : 0);
    SampledCloud out;
    out.points.resize(rows * 3);
    if (normals) out.normals.resize(rows * 3);
    if (covs) out.covs.resize(rows * 9);
    int64_t k = 0;
    withFeatureHandle(device, [&](reg_handle* h) {
        return reg_voxel_down_sample(h, points, normals, covs, n, 0, voxelSize, out.points.data(),
                                     normals ? out.normals.data() : nullptr, covs ? out.covs.data() : nullptr, &k);
    });
    out.points.resize((size_t)k * 3);
    if (normals) out.normals.resize((size_t)k * 3);
    if (covs) out.covs.resize((size_t)k * 9);
    return out;
}
inline SampledCloud randomDownSample(const double* points, const double* normals, const double* covs, int64_t n,
                                     double ratio, uint64_t seed = 0, int device = 0) {
    const size_t rows = (size_t)(n > 0 ? n : 0);
    SampledCloud out;
    out.indices.resize(rows);
    if (points) out.points.resize(rows * 3);
    if (normals) out.normals.resize(rows * 3);
    if (covs) out.covs.resize(rows * 9);
    int64_t k = 0;
    withFeatureHandle(device, [&](reg_handle* h) {
        return reg_random_down_sample(h, points, normals, covs, n, 0, ratio, seed, out.indices.data(),
                                      points ? out.points.data() : nullptr, normals ? out.normals.data() : nullptr,
                                      covs ? out.covs.data() : nullptr, &k);
    });
    out.indices.resize((size_t)k);
    if (points) out.points.resize((size_t)k * 3);
    if (normals) out.normals.resize((size_t)k * 3);
    if (covs) out.covs.resize((size_t)k * 9);
    return out;
}

// RegistrationRANSACBasedOnCorrespondence with TransformationEstimationPointToPoint(false), the edge-length and the
// distance checker (PlaceRecognition.cpp:78-91) on the device: `source` (n x 3) and `target` (m x 3) doubles and the
// interleaved (source, target) pairs of matchFeatures in host memory.  A checker threshold <= 0 switches it off.
// Deterministic for a given seed (include/o3dslam_reg.h, reg_ransac_correspondences).
struct RansacResult {
    std::array<double, 16> transformation{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};   // column-major
    double fitness = 0.0, inlierRmse = 0.0;
    std::vector<int32_t> correspondenceSet;   // interleaved (source, target) inlier pairs
    int64_t iterations = 0, validated = 0, bestIteration = -1;
};
inline RansacResult ransacFromCorrespondences(const double* source, int64_t n, const double* target, int64_t m,
                                              const std::vector<int32_t>& corres, double maxCorrespondenceDistance = 0.75,
                                              int ransacN = 3, int64_t maxIteration = 1000000, double confidence = 0.99,
                                              double checkerDistance = 0.75, double checkerEdgeLength = 0.5,
                                              uint64_t seed = 0, int device = 0) {
    RansacResult out;
    const int64_t k = (int64_t)(corres.size() / 2);
    if (k == 0) return out;
    reg_ransac_params p{};
    p.struct_size = (int32_t)sizeof(p);
    p.ransac_n = ransacN;
    p.max_iteration = maxIteration;
    p.confidence = confidence;
    p.max_correspondence_distance = maxCorrespondenceDistance;
    p.distance_threshold = checkerDistance;
    p.edge_similarity = checkerEdgeLength;
    p.seed = seed;
    reg_ransac_result r{};
    r.struct_size = (int32_t)sizeof(r);
    out.correspondenceSet.resize((size_t)(2 * k));
    withFeatureHandle(device, [&](reg_handle* h) {
        return reg_ransac_correspondences(h, source, n, target, m, corres.data(), k, 0, &p, &r, out.correspondenceSet.data(),
                                          nullptr);
    });
    std::copy(r.T, r.T + 16, out.transformation.begin());
    out.fitness = r.fitness;
    out.inlierRmse = r.inlier_rmse;
    out.correspondenceSet.resize((size_t)(2 * r.n_inliers));
    out.iterations = r.n_iterations;
    out.validated = r.n_validated;
    out.bestIteration = r.best_iteration;
    return out;
}

// SurfaceNormalDataPointsFilter (DataPointsFilters/SurfaceNormal.cpp:152-252) on the device: exact k-NN (the point
// itself included) + PCA.  Outputs are written to caller-owned arrays laid out like the `normals` (3 x N),
// `eigValues` (3 x N, ascending == sortEigen) and `matchedIds` (knn x N) descriptors.
class SurfaceNormalFilter {
public:
    unsigned knn = 5;                                             // SurfaceNormal.h:68
    float maxDist = std::numeric_limits<float>::infinity();      // SurfaceNormal.h:69
    bool smoothNormals = false;                                   // SurfaceNormal.h:76, SurfaceNormal.cpp:259-283
    bool orientTowardsViewpoint = false;                          // CloudRegistration.cpp:37 (camera location)
    std::array<float, 3> viewpoint{{0.f, 0.f, 0.f}};

    SurfaceNormalFilter() = default;
    ~SurfaceNormalFilter() { if (h_) reg_destroy(h_); }
    SurfaceNormalFilter(const SurfaceNormalFilter&) = delete;
    SurfaceNormalFilter& operator=(const SurfaceNormalFilter&) = delete;

    // optional outputs by the reference's descriptor names: eigValues 3xN (ascending), matchedIds knn x N, densities N,
    // meanDists N, eigVectors 9xN; covariances6 {xx xy xz yy yz zz} for the GICP operator
    void compute(const DataPointsView& cloud, float* normals, float* eigValues = nullptr, int32_t* matchedIds = nullptr,
                 float* covariances6 = nullptr, bool regularisedCovariances = false, float* densities = nullptr,
                 float* meanDists = nullptr, float* eigVectors = nullptr) {
        if (!h_) {
            reg_params p;
            reg_default_params(&p);
            reg_status s = reg_create(&p, &h_);
            if (s != REG_OK) {
                std::string msg = h_ ? reg_last_error(h_) : "reg_create failed";
                if (h_) { reg_destroy(h_); h_ = nullptr; }
                throw DeviceError(msg);
            }
        }
        if (cloud.getNbPoints() == 0) throw std::runtime_error("The point cloud is empty.");
        reg_normals_out out{};
        out.normals = normals;
        out.eigvals = eigValues;
        out.covs = covariances6;
        std::vector<int32_t> own_ids;   // smoothNormals needs the neighbour lists even when the caller does not ask for them
        if (smoothNormals && !matchedIds && !cloud.on_device) {
            own_ids.resize((size_t)cloud.n * knn);
            matchedIds = own_ids.data();
        }
        if (smoothNormals && !matchedIds)
            throw InvalidParameter("smoothNormals on device buffers needs a matchedIds buffer (n x knn int32)");
        out.ids = matchedIds;
        out.densities = densities;
        out.mean_dists = meanDists;
        out.eigvecs = eigVectors;
        const reg_status s = reg_estimate_normals(h_, cloud.features, cloud.feature_stride, cloud.n,
                                                  cloud.on_device ? 1 : 0, (int)knn, maxDist,
                                                  orientTowardsViewpoint ? viewpoint.data() : nullptr,
                                                  regularisedCovariances ? 1 : 0, &out, nullptr);
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(reg_last_error(h_));
        if (s == REG_MISSING_FIELD) throw InvalidField(reg_last_error(h_));
        if (s == REG_DEVICE_ERROR) throw DeviceError(reg_last_error(h_));
        if (s != REG_OK) throw std::runtime_error(reg_last_error(h_));
        if (smoothNormals) {
            const reg_status t = reg_smooth_normals(h_, normals, matchedIds, cloud.n, (int)knn, cloud.on_device ? 1 : 0, nullptr);
            if (t == REG_DEVICE_ERROR) throw DeviceError(reg_last_error(h_));
            if (t != REG_OK) throw std::runtime_error(reg_last_error(h_));
        }
    }

private:
    reg_handle* h_ = nullptr;
};

// Base of the two data-point filter wrappers below: owns one handle, maps statuses to the reference's exceptions.
class DeviceFilterBase {
public:
    DeviceFilterBase() = default;
    ~DeviceFilterBase() { if (h_) reg_destroy(h_); }
    DeviceFilterBase(const DeviceFilterBase&) = delete;
    DeviceFilterBase& operator=(const DeviceFilterBase&) = delete;

protected:
    reg_handle* handle() {
        if (!h_) {
            reg_params p;
            reg_default_params(&p);
            reg_status s = reg_create(&p, &h_);
            if (s != REG_OK) {
                std::string msg = h_ ? reg_last_error(h_) : "reg_create failed";
                if (h_) { reg_destroy(h_); h_ = nullptr; }
                throw DeviceError(msg);
            }
        }
        return h_;
    }
    void check(reg_status s) const {
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(reg_last_error(h_));
        if (s == REG_DEVICE_ERROR) throw DeviceError(reg_last_error(h_));
        if (s != REG_OK) throw std::runtime_error(reg_last_error(h_));
    }
    reg_handle* h_ = nullptr;
};

// SamplingSurfaceNormalDataPointsFilter (DataPointsFilters/SamplingSurfaceNormal.cpp) on the device
// (reg_sampling_surface_normal; determinism contract in include/o3dslam_reg.h).  Every output holds n rows of capacity;
// returns the number of rows written.
class SamplingSurfaceNormalFilter : public DeviceFilterBase {
public:
    reg_ssn_params params;
    SamplingSurfaceNormalFilter() { reg_default_ssn_params(&params); }

    int64_t compute(const DataPointsView& cloud, const reg_ssn_out& out, int64_t* unfitPointsCount = nullptr) {
        int64_t m = 0;
        check(reg_sampling_surface_normal(handle(), cloud.features, cloud.feature_stride, cloud.n, cloud.on_device ? 1 : 0,
                                          &params, &out, &m, unfitPointsCount));
        return m;
    }
};

// OctreeGridDataPointsFilter (DataPointsFilters/OctreeGrid.cpp) on the device (reg_octree_grid; determinism contract
// and the documented sampler deviation in include/o3dslam_reg.h).  normals (n x 3) and covs6 (n x 6) may be NULL and are
// carried to out.normals / out.covs.  Every output holds n rows of capacity; returns the number of rows written.
class OctreeGridFilter : public DeviceFilterBase {
public:
    reg_octree_params params;
    OctreeGridFilter() { reg_default_octree_params(&params); }

    int64_t compute(const DataPointsView& cloud, const reg_octree_out& out, const float* normals = nullptr,
                    const float* covs6 = nullptr) {
        int64_t m = 0;
        check(reg_octree_grid(handle(), cloud.features, cloud.feature_stride, normals, covs6, cloud.n,
                              cloud.on_device ? 1 : 0, &params, &out, &m));
        return m;
    }
};

// The reading-side chain of reg_filter_points (MaxDist, MinDist, BoundingBox, DistanceLimit, RemoveNaN,
// MaxQuantileOnAxis, FixStepSampling, Identity), applied in order.  Returns the number of points kept.
class PointFilterChain : public DeviceFilterBase {
public:
    std::vector<reg_point_filter> filters;

    int64_t compute(const DataPointsView& cloud, float* out_xyz, int32_t* out_idx = nullptr, const float* normals = nullptr,
                    float* out_normals = nullptr, const float* covs6 = nullptr, float* out_covs6 = nullptr) {
        int64_t m = 0;
        check(reg_filter_points(handle(), cloud.features, cloud.feature_stride, normals, covs6, cloud.n,
                                cloud.on_device ? 1 : 0, filters.data(), (int)filters.size(), out_xyz, out_normals,
                                out_covs6, out_idx, &m));
        return m;
    }
};

// The descriptor-carrying chain of reg_filter_cloud: the filters of PointFilterChain plus ObservationDirection,
// OrientNormals, Shadow, SimpleSensorNoise, IncidenceAngle, CutAtDescriptorThreshold and MaxDensity, over xyz and up to
// REG_MAX_FIELDS descriptor fields (include/o3dslam_reg.h gives each filter's contract and which fields it names).
// add() returns the index of a field: `in` NULL for one the chain creates, `out` with n rows of capacity or NULL.
// A filter that reads a field which does not exist at its place throws InvalidField, as the reference does.
class CloudFilterChain : public DeviceFilterBase {
public:
    std::vector<reg_field> fields;
    std::vector<reg_cloud_filter> filters;

    int add(const float* in, float* out, int span) {
        reg_field f{};
        f.in = in;
        f.out = out;
        f.span = span;
        fields.push_back(f);
        return (int)fields.size() - 1;
    }
    // a record with struct_size set and no field named; fill base.type and what the type reads
    static reg_cloud_filter filter(int type) {
        reg_cloud_filter c{};
        c.struct_size = (int32_t)sizeof(reg_cloud_filter);
        c.base.type = type;
        c.field_a = c.field_b = c.field_out = -1;
        c.seed = 1;
        return c;
    }
    int64_t compute(const DataPointsView& cloud, float* out_xyz, int32_t* out_idx = nullptr) {
        int64_t m = 0;
        check(reg_filter_cloud(handle(), cloud.features, cloud.feature_stride, cloud.n, cloud.on_device ? 1 : 0,
                               fields.data(), (int)fields.size(), filters.data(), (int)filters.size(), out_xyz, out_idx,
                               &m));
        return m;
    }
};

// VoxelGridDataPointsFilter with useCentroid 1 (reg_voxel_grid; contract in include/o3dslam_reg.h): one output row per
// occupied voxel, ascending by its first member's index; `fields` as for CloudFilterChain (every field with `in` set).
class VoxelGridFilter : public DeviceFilterBase {
public:
    reg_voxel_grid_params params;
    std::vector<reg_field> fields;
    VoxelGridFilter() { reg_default_voxel_grid_params(&params); }

    int64_t compute(const DataPointsView& cloud, float* out_xyz, int32_t* out_idx = nullptr) {
        int64_t m = 0;
        check(reg_voxel_grid(handle(), cloud.features, cloud.feature_stride, cloud.n, cloud.on_device ? 1 : 0,
                             fields.data(), (int)fields.size(), &params, out_xyz, out_idx, &m));
        return m;
    }
};

// o3d_slam::VoxelizedPointCloud -- the dense map of a submap -- resident on the device (reg_dense_map; contract in
// include/o3dslam_reg.h).  RAII, move-only.  The map owns a handle that only lends its stream and working storage, and
// destroys itself before it.  Clouds are Open3D's fp64 arrays in host memory (n x 3 doubles each; normals / colors may be
// nullptr); transforms are column-major double[16] (Eigen::Matrix4d::data(), nullptr: identity).  Departures from the
// reference: voxels are exported in ascending (z, y, x) key order; a non-finite point or a voxel index outside +-(2^20 - 1)
// throws InvalidParameter and leaves the map unchanged; the carve's loops are bounded.  Reproduced oddity: transform() maps
// the position and normal SUMS by R S + t and keeps the keys, as Voxel.cpp:49-64 does.
class DenseMap {
public:
    struct Cloud {
        std::vector<double> points, normals, colors;
        std::vector<int32_t> keys, counts;   // keys: (x, y, z) per voxel
        int64_t size() const { return (int64_t)(points.size() / 3); }
    };

    explicit DenseMap(double voxelSize, int device = 0) {
        reg_params p;
        reg_default_params(&p);
        p.cost = REG_COST_O3D_P2P;   // no field requirements
        p.device = device;
        reg_status s = reg_create(&p, &h_);
        if (s == REG_OK) s = reg_dense_map_create(h_, voxelSize, &m_);
        if (s != REG_OK) {
            const std::string msg = h_ ? reg_last_error(h_) : "reg_create rejected the parameters";
            release();
            raise(s, msg);
        }
    }
    ~DenseMap() { release(); }
    DenseMap(const DenseMap&) = delete;
    DenseMap& operator=(const DenseMap&) = delete;
    DenseMap(DenseMap&& o) noexcept : h_(o.h_), m_(o.m_) { o.h_ = nullptr, o.m_ = nullptr; }
    DenseMap& operator=(DenseMap&& o) noexcept {
        if (this != &o) {
            release();
            h_ = o.h_, m_ = o.m_;
            o.h_ = nullptr, o.m_ = nullptr;
        }
        return *this;
    }

    // VoxelizedPointCloud::insert(transform(T, cloud)); returns the number of new voxels
    int64_t insert(const double* points, const double* normals, const double* colors, int64_t n, const double* T = nullptr) {
        int64_t nVoxels = 0, nNew = 0;
        check(reg_dense_map_insert(m_, points, normals, colors, n, 0, T, &nVoxels, &nNew));
        return nNew;
    }
    // Submap.cpp:99-106: dense-map cropper, ColorRangeCropper, transform, insert; returns the points that passed the croppers
    int64_t insertScan(const double* points, const double* normals, const double* colors, int64_t n,
                       const reg_dense_scan_params& params, const double* mapToRangeSensor) {
        int64_t nInserted = 0, nVoxels = 0;
        check(reg_dense_map_insert_scan(m_, points, normals, colors, n, 0, &params, mapToRangeSensor, &nInserted, &nVoxels));
        return nInserted;
    }
    // getKeysOfCarvedPoints + removeKey (helpers.cpp:360-390, Submap.cpp:153-156): the erased keys, (x, y, z) per voxel
    std::vector<int32_t> carve(const double* scan, int64_t n, const double sensor[3], const reg_dense_carve_params& params) {
        std::vector<int32_t> keys((size_t)info().n_voxels * 3);
        int64_t k = 0;
        check(reg_dense_map_carve(m_, scan, n, 0, sensor, &params, keys.data(), &k));
        keys.resize((size_t)k * 3);
        return keys;
    }
    // Submap::carve for the dense map (Submap.cpp:146-157) in one call: transform by T (nullptr: the scan as given, the
    // reference's choice), removeDuplicatePointsWithinSameVoxels, getKeysOfCarvedPoints, removeKey; the erased keys
    std::vector<int32_t> carveScan(const double* scan, int64_t n, const double sensor[3], const reg_dense_carve_params& params,
                                   const double* T = nullptr) {
        std::vector<int32_t> keys((size_t)info().n_voxels * 3);
        int64_t k = 0;
        check(reg_dense_map_carve_scan(m_, scan, n, 0, sensor, &params, T, keys.data(), &k));
        keys.resize((size_t)k * 3);
        return keys;
    }
    void transform(const double T[16]) { check(reg_dense_map_transform(m_, T)); }
    std::array<double, 3> center() {
        std::array<double, 3> c{};
        check(reg_dense_map_center(m_, c.data()));
        return c;
    }
    void clear() { check(reg_dense_map_clear(m_)); }
    reg_dense_map_info info() const {
        reg_dense_map_info i{};
        i.struct_size = (int32_t)sizeof(i);
        check(reg_dense_map_get_info(m_, &i));
        return i;
    }
    int64_t size() const { return info().n_voxels; }
    bool empty() const { return size() == 0; }
    // toPointCloud (+ keys and counts)
    Cloud exportCloud(bool wantKeys = false, bool wantCounts = false) {
        const reg_dense_map_info i = info();
        const size_t rows = (size_t)i.n_voxels;
        Cloud out;
        out.points.resize(rows * 3);
        if (i.has_normals) out.normals.resize(rows * 3);
        if (i.has_colors) out.colors.resize(rows * 3);
        if (wantKeys) out.keys.resize(rows * 3);
        if (wantCounts) out.counts.resize(rows);
        int64_t k = 0;
        check(reg_dense_map_export(m_, 0, out.points.data(), i.has_normals ? out.normals.data() : nullptr,
                                   i.has_colors ? out.colors.data() : nullptr, wantKeys ? out.keys.data() : nullptr,
                                   wantCounts ? out.counts.data() : nullptr, i.n_voxels, &k));
        return out;
    }
    // removeDuplicatePointsWithinSameVoxels (Voxel.cpp:162-191): ascending indices of the first point of every voxel
    std::vector<int32_t> dedupVoxels(const double* points, int64_t n, double voxelSize) {
        std::vector<int32_t> idx((size_t)(n > 0 ? n : 0));
        int64_t k = 0;
        check(reg_dedup_voxels(h_, points, n, 0, voxelSize, idx.data(), &k));
        idx.resize((size_t)k);
        return idx;
    }
    reg_dense_map* map() const { return m_; }
    reg_handle* handle() const { return h_; }

private:
    static void raise(reg_status s, const std::string& msg) {
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
        if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
        throw std::runtime_error(msg);
    }
    void check(reg_status s) const {
        if (s != REG_OK) raise(s, reg_last_error(h_));
    }
    void release() {
        if (m_) reg_dense_map_destroy(m_);   // the map goes before its handle
        if (h_) reg_destroy(h_);
        m_ = nullptr, h_ = nullptr;
    }
    reg_handle* h_ = nullptr;
    reg_dense_map* m_ = nullptr;
};

// o3d_slam::Submap's scan-matching map (mapCloud_) resident on the device (reg_map_cloud; contract in
// include/o3dslam_reg.h): insertScan (Submap.cpp:39-96: carve, append, setPose, voxelise), setAsReference (cropSubmap +
// initReference), transform, centre, export.  RAII, move-only.  The map lives on a registration handle: one it creates from
// `reg` and owns, or the caller's (borrowed; the map must go before it) -- setAsReference installs the patch on that handle,
// which handle() hands to the registration calls.  Clouds are Open3D's fp64 arrays in host memory (n x 3 doubles; covariances
// n x 9); transforms are column-major double[16].  Followed from the reference: the carve runs when nScansInsertedMap_ %
// carve_every_n_scans == 1 and uses the cropper pose of the previous insert.  Departures: the field set is fixed at
// construction and a scan with other fields throws InvalidParameter; voxels come in ascending (z, y, x) order.
class MapCloud {
public:
    struct Cloud {
        std::vector<double> points, normals, covariances;
        int64_t size() const { return (int64_t)(points.size() / 3); }
    };

    MapCloud(const reg_map_cloud_params& params, const reg_params& reg) : owns_(true) {
        reg_status s = reg_create(&reg, &h_);
        if (s == REG_OK) s = reg_map_cloud_create(h_, &params, &m_);
        if (s != REG_OK) {
            const std::string msg = h_ ? reg_last_error(h_) : "reg_create rejected the parameters";
            release();
            raise(s, msg);
        }
    }
    MapCloud(reg_handle* handle, const reg_map_cloud_params& params) : h_(handle), owns_(false) {
        const reg_status s = reg_map_cloud_create(h_, &params, &m_);
        if (s != REG_OK) raise(s, h_ ? reg_last_error(h_) : "no handle");
    }
    ~MapCloud() { release(); }
    MapCloud(const MapCloud&) = delete;
    MapCloud& operator=(const MapCloud&) = delete;
    MapCloud(MapCloud&& o) noexcept : h_(o.h_), m_(o.m_), owns_(o.owns_) { o.h_ = nullptr, o.m_ = nullptr; }
    MapCloud& operator=(MapCloud&& o) noexcept {
        if (this != &o) {
            release();
            h_ = o.h_, m_ = o.m_, owns_ = o.owns_;
            o.h_ = nullptr, o.m_ = nullptr;
        }
        return *this;
    }

    // the isUseInitialMap_ branch (Submap.cpp:47-52); returns the rows of the map
    int64_t set(const double* points, const double* normals, const double* covariances, int64_t n, double voxelSize) {
        check(reg_map_cloud_set(m_, points, normals, covariances, n, 0, voxelSize));
        return size();
    }
    // Submap::insertScan (Submap.cpp:54-95)
    reg_map_cloud_insert_result insertScan(const double* rawScan, int64_t nRaw, const double* points, const double* normals,
                                           const double* covariances, int64_t n, const double mapToRangeSensor[16],
                                           bool isPerformCarving = true) {
        reg_map_cloud_insert_result r{};
        r.struct_size = (int32_t)sizeof(r);
        check(reg_map_cloud_insert_scan(m_, rawScan, nRaw, points, normals, covariances, n, 0, mapToRangeSensor,
                                        isPerformCarving ? 1 : 0, &r));
        return r;
    }
    // cropSubmap + open3dToPointmatcher + initReference on handle(); returns the rows of the patch
    int64_t setAsReference(const reg_crop* crop) {
        int64_t kept = 0;
        check(reg_map_cloud_set_target(m_, crop, &kept));
        return kept;
    }
    void transform(const double T[16]) { check(reg_map_cloud_transform(m_, T)); }
    std::array<double, 3> center() {
        std::array<double, 3> c{};
        check(reg_map_cloud_center(m_, c.data()));
        return c;
    }
    void clear() { check(reg_map_cloud_clear(m_)); }
    reg_map_cloud_info info() const {
        reg_map_cloud_info i{};
        i.struct_size = (int32_t)sizeof(i);
        check(reg_map_cloud_get_info(m_, &i));
        return i;
    }
    int64_t size() const { return info().n_rows; }
    bool empty() const { return size() == 0; }
    Cloud exportCloud() {
        const reg_map_cloud_info i = info();
        const size_t rows = (size_t)i.n_rows;
        Cloud out;
        out.points.resize(rows * 3);
        if (i.has_normals) out.normals.resize(rows * 3);
        if (i.has_covariances) out.covariances.resize(rows * 9);
        int64_t k = 0;
        check(reg_map_cloud_export(m_, 0, out.points.data(), i.has_normals ? out.normals.data() : nullptr,
                                   i.has_covariances ? out.covariances.data() : nullptr, i.n_rows, &k));
        return out;
    }
    reg_map_cloud* map() const { return m_; }
    reg_handle* handle() const { return h_; }

private:
    static void raise(reg_status s, const std::string& msg) {
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
        if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
        throw std::runtime_error(msg);
    }
    void check(reg_status s) const {
        if (s != REG_OK) raise(s, reg_last_error(h_));
    }
    void release() {
        if (m_) reg_map_cloud_destroy(m_);   // the map goes before its handle
        if (h_ && owns_) reg_destroy(h_);
        m_ = nullptr, h_ = nullptr;
    }
    reg_handle* h_ = nullptr;
    reg_map_cloud* m_ = nullptr;
    bool owns_ = false;
};

// reg_undistort_scan on host arrays through `handle` (contract in include/o3dslam_reg.h):
// ConstantVelocityMotionCompensation::undistortInputPointCloud for given velocities.  Points are n x 3 doubles.
inline std::vector<double> undistortScan(reg_handle* handle, const double* points, int64_t n, const reg_undistort_params& params) {
    std::vector<double> out((size_t)n * 3);
    const reg_status s = reg_undistort_scan(handle, points, n, 0, &params, out.data());
    if (s != REG_OK) {
        const std::string msg = handle ? reg_last_error(handle) : "no handle";
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
        if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
        throw std::runtime_error(msg);
    }
    return out;
}

// ConstantVelocityMotionCompensation::estimateLinearAndAngularVelocity (MotionCompensation.cpp:32-57) over a pose list, oldest
// first, written as the reference evidently intends it (its own const buffer returns the latest pose for every offset, so it
// can only throw): from the latest pose and the one numPoses before it, dT = start^-1 * finish,
// linear = dT.translation / (dt + 1e-6), angularRpy = roll / pitch / yaw of dT.rotation / (dt + 1e-6).  Both are zero while
// the list holds no more than numPoses poses or already reaches stampNs.  Host arithmetic; poses are column-major double[16],
// rigid; stamps are nanoseconds.  The result fills reg_undistort_params::linear_velocity / angular_velocity_rpy.
struct StampedPose {
    int64_t stampNs;
    std::array<double, 16> pose;
};
inline void estimateLinearAndAngularVelocity(const std::vector<StampedPose>& buffer, int64_t stampNs, int numPoses,
                                             double linear[3], double angularRpy[3]) {
    for (int k = 0; k < 3; ++k) linear[k] = angularRpy[k] = 0.0;
    if (numPoses < 1) throw InvalidParameter("numPosesVelocityEstimation_ must be >= 1");
    if (buffer.size() <= (size_t)numPoses || !(buffer.back().stampNs < stampNs)) return;
    const StampedPose &fin = buffer.back(), &start = buffer[buffer.size() - 1 - (size_t)numPoses];
    const double dt = (double)(fin.stampNs - start.stampNs) * 1e-9;
    if (!(dt > 0.0)) throw std::runtime_error("dt should be > 0!!!!");
    const double *A = start.pose.data(), *B = fin.pose.data();   // m(r, c) = pose[4 c + r]; start^-1 = (R^T, -R^T t)
    double R[9], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[3 * r + c] = A[4 * r] * B[4 * c] + A[4 * r + 1] * B[4 * c + 1] + A[4 * r + 2] * B[4 * c + 2];
        t[r] = A[4 * r] * (B[12] - A[12]) + A[4 * r + 1] * (B[13] - A[13]) + A[4 * r + 2] * (B[14] - A[14]);
    }
    // toRPY of R = Rz(yaw) Ry(pitch) Rx(roll) (math.hpp:30-42 reads the same three angles off the quaternion)
    const double rpy[3] = {std::atan2(R[7], R[8]), std::asin(std::max(-1.0, std::min(1.0, -R[6]))), std::atan2(R[3], R[0])};
    for (int k = 0; k < 3; ++k) linear[k] = t[k] / (dt + 1e-6), angularRpy[k] = rpy[k] / (dt + 1e-6);
}

// reg_covariances_from_normals on host arrays through `handle` (contract in include/o3dslam_reg.h): the
// covariances Open3D's GeneralizedICP derives from normals.  n x 3 doubles in, n x 9 doubles out.
inline std::vector<double> covariancesFromNormals(reg_handle* handle, const double* normals, int64_t n, double epsilon = 1e-3) {
    std::vector<double> out((size_t)(n > 0 ? n : 0) * 9);
    const reg_status s = reg_covariances_from_normals(handle, normals, n, 0, epsilon, out.data());
    if (s != REG_OK) {
        const std::string msg = handle ? reg_last_error(handle) : "no handle";
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
        if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
        throw std::runtime_error(msg);
    }
    return out;
}

// o3d_slam::LidarOdometry over reg_odometry (Odometry.cpp): the previous pre-processed cloud stays on the device
// between scans.  RAII, move-only.  The object lives on a registration handle: one it creates from `reg` and owns, or the
// caller's (borrowed; the object must go before it).  `reg` selects the operator: REG_COST_GICP, REG_COST_O3D_P2PL or
// REG_COST_O3D_P2P, configured as the Open3D operators are (use_trimmed = 0; gicp_stop_rule = 1 for GICP).  The buffer of
// stamped poses is the caller's side of getOdomToRangeSensor: addRangeScan appends (stamp, cumulative) whenever the library
// says pose_updated.  Clouds are host arrays (n x 3 doubles); stamps are nanoseconds; poses column-major double[16].
class LidarOdometry {
public:
    struct Cloud {
        std::vector<double> points, normals, covariances;
        int64_t size() const { return (int64_t)(points.size() / 3); }
    };

    LidarOdometry(const reg_odometry_params& params, const reg_params& reg) : owns_(true) {
        reg_status s = reg_create(&reg, &h_);
        if (s == REG_OK) s = reg_odometry_create(h_, &params, &o_);
        if (s != REG_OK) {
            const std::string msg = h_ ? reg_last_error(h_) : "reg_create rejected the parameters";
            release();
            raise(s, msg);
        }
    }
    LidarOdometry(reg_handle* handle, const reg_odometry_params& params) : h_(handle), owns_(false) {
        const reg_status s = reg_odometry_create(h_, &params, &o_);
        if (s != REG_OK) raise(s, h_ ? reg_last_error(h_) : "no handle");
    }
    ~LidarOdometry() { release(); }
    LidarOdometry(const LidarOdometry&) = delete;
    LidarOdometry& operator=(const LidarOdometry&) = delete;
    LidarOdometry(LidarOdometry&& o) noexcept : buffer_(std::move(o.buffer_)), last_(o.last_), h_(o.h_), o_(o.o_), owns_(o.owns_) {
        o.h_ = nullptr, o.o_ = nullptr;
    }
    LidarOdometry& operator=(LidarOdometry&& o) noexcept {
        if (this != &o) {
            release();
            buffer_ = std::move(o.buffer_), last_ = o.last_, h_ = o.h_, o_ = o.o_, owns_ = o.owns_;
            o.h_ = nullptr, o.o_ = nullptr;
        }
        return *this;
    }

    // addRangeScan (Odometry.cpp:29-84); normals may be null.  lastResult() keeps the counts, the transform and the times.
    bool addRangeScan(const double* points, const double* normals, int64_t n, int64_t stampNs) {
        reg_odometry_result r{};
        r.struct_size = (int32_t)sizeof(r);
        check(reg_odometry_add_scan(o_, points, normals, n, 0, stampNs, &r));
        last_ = r;
        if (r.pose_updated) {
            StampedPose p{stampNs, {}};
            std::copy(r.cumulative, r.cumulative + 16, p.pose.begin());
            buffer_.push_back(p);
        }
        return r.accepted != 0;
    }
    // false (and nothing changes) while an earlier initial transform is still pending
    bool setInitialTransform(const double T[16]) {
        int32_t applied = 0;
        check(reg_odometry_set_initial_transform(o_, T, &applied));
        return applied != 0;
    }
    void clear() {
        check(reg_odometry_clear(o_));
        buffer_.clear();
    }
    reg_odometry_info info() const {
        reg_odometry_info i{};
        i.struct_size = (int32_t)sizeof(i);
        check(reg_odometry_get_info(o_, &i));
        return i;
    }
    // getPreProcessedCloud: sized from the library's own row count, which the export checks again
    Cloud getPreProcessedCloud() {
        const reg_odometry_info i = info();
        const size_t rows = (size_t)i.n_rows;
        Cloud out;
        out.points.resize(rows * 3);
        if (i.has_normals) out.normals.resize(rows * 3);
        if (i.has_covariances) out.covariances.resize(rows * 9);
        int64_t k = 0;
        check(reg_odometry_export_cloud(o_, 0, out.points.data(), i.has_normals ? out.normals.data() : nullptr,
                                        i.has_covariances ? out.covariances.data() : nullptr, i.n_rows, &k));
        return out;
    }
    const std::vector<StampedPose>& getBuffer() const { return buffer_; }
    bool hasProcessedMeasurements() const { return !buffer_.empty(); }
    const reg_odometry_result& lastResult() const { return last_; }
    reg_odometry* odometry() const { return o_; }
    reg_handle* handle() const { return h_; }

private:
    static void raise(reg_status s, const std::string& msg) {
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
        if (s == REG_MISSING_FIELD) throw InvalidField(msg);
        if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
        throw std::runtime_error(msg);
    }
    void check(reg_status s) const {
        if (s != REG_OK) raise(s, reg_last_error(h_));
    }
    void release() {
        if (o_) reg_odometry_destroy(o_);   // the object goes before its handle
        if (h_ && owns_) reg_destroy(h_);
        o_ = nullptr, h_ = nullptr;
    }
    std::vector<StampedPose> buffer_;
    reg_odometry_result last_{};
    reg_handle* h_ = nullptr;
    reg_odometry* o_ = nullptr;
    bool owns_ = false;
};

// Open3D's PoseGraph + GlobalOptimization over reg_pose_graph (OptimizationProblem.cpp:25-44).  RAII, move-only,
// on a caller's registration handle (borrowed; the object must go before it).  Every matrix is ROW-major double: poses and
// edge transformations 16 per item, information matrices 36.  Parity with Open3D 0.15.1 is unpinned (include/o3dslam_reg.h).
class PoseGraph {
public:
    struct Edge {
        int32_t source = 0, target = 0;
        std::array<double, 16> transformation{};
        std::array<double, 36> information{};
        bool uncertain = false;
        double confidence = 1.0;
    };
    struct Graph {
        std::vector<std::array<double, 16>> poses;
        std::vector<int32_t> source, target, ids;   // ids: the edge's index in the list set() received
        std::vector<double> confidence;
    };

    static reg_pose_graph_params defaults() {
        reg_pose_graph_params p;
        reg_default_pose_graph_params(&p);
        return p;
    }
    explicit PoseGraph(reg_handle* handle, const reg_pose_graph_params& params = defaults()) : h_(handle) {
        const reg_status s = reg_pose_graph_create(h_, &params, &g_);
        if (s != REG_OK) raise(s, h_ ? reg_last_error(h_) : "no handle");
    }
    ~PoseGraph() { release(); }
    PoseGraph(const PoseGraph&) = delete;
    PoseGraph& operator=(const PoseGraph&) = delete;
    PoseGraph(PoseGraph&& o) noexcept : h_(o.h_), g_(o.g_) { o.h_ = nullptr, o.g_ = nullptr; }
    PoseGraph& operator=(PoseGraph&& o) noexcept {
        if (this != &o) {
            release();
            h_ = o.h_, g_ = o.g_;
            o.h_ = nullptr, o.g_ = nullptr;
        }
        return *this;
    }

    void set(const std::vector<std::array<double, 16>>& poses, const std::vector<Edge>& edges) {
        const size_t E = edges.size();
        std::vector<int32_t> src(E), tgt(E), unc(E);
        std::vector<double> X(E * 16), info(E * 36), conf(E);
        for (size_t e = 0; e < E; ++e) {
            src[e] = edges[e].source, tgt[e] = edges[e].target, unc[e] = edges[e].uncertain, conf[e] = edges[e].confidence;
            std::copy(edges[e].transformation.begin(), edges[e].transformation.end(), X.begin() + 16 * e);
            std::copy(edges[e].information.begin(), edges[e].information.end(), info.begin() + 36 * e);
        }
        check(reg_pose_graph_set(g_, poses.empty() ? nullptr : poses[0].data(), (int64_t)poses.size(), src.data(), tgt.data(),
                                 X.data(), info.data(), unc.data(), conf.data(), (int64_t)E));
    }
    void clear() { check(reg_pose_graph_clear(g_)); }
    // one Levenberg-Marquardt pass on the graph as it stands
    reg_pose_graph_result optimize() {
        reg_pose_graph_result r{};
        r.struct_size = (int32_t)sizeof(r);
        check(reg_pose_graph_optimize(g_, &r));
        return r;
    }
    // GlobalOptimization: pass, prune, pass, prune, reference compensation
    std::array<reg_pose_graph_result, 2> globalOptimize() {
        std::array<reg_pose_graph_result, 2> r{};
        r[0].struct_size = r[1].struct_size = (int32_t)sizeof(reg_pose_graph_result);
        check(reg_pose_graph_global_optimize(g_, r.data()));
        return r;
    }
    reg_pose_graph_info info() const {
        reg_pose_graph_info i{};
        i.struct_size = (int32_t)sizeof(i);
        check(reg_pose_graph_get_info(g_, &i));
        return i;
    }
    // sized from the library's own counts, which the getters check again
    Graph get() {
        const reg_pose_graph_info i = info();
        Graph out;
        out.poses.resize((size_t)i.n_nodes);
        out.source.resize((size_t)i.n_edges), out.target.resize((size_t)i.n_edges), out.ids.resize((size_t)i.n_edges);
        out.confidence.resize((size_t)i.n_edges);
        int64_t k = 0;
        check(reg_pose_graph_get(g_, i.n_nodes, out.poses.empty() ? nullptr : out.poses[0].data(), i.n_edges, out.source.data(),
                                 out.target.data(), out.confidence.data(), &k));
        if (i.n_edges > 0) check(reg_pose_graph_get_edge_ids(g_, i.n_edges, out.ids.data()));
        return out;
    }
    reg_pose_graph* graph() const { return g_; }
    reg_handle* handle() const { return h_; }

private:
    static void raise(reg_status s, const std::string& msg) {
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
        if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
        throw std::runtime_error(msg);   // REG_BAD_TRANSFORM: a pivot of the factorisation (the message names its row)
    }
    void check(reg_status s) const {
        if (s != REG_OK) raise(s, reg_last_error(h_));
    }
    void release() {
        if (g_) reg_pose_graph_destroy(g_);   // the object goes before its handle
        g_ = nullptr, h_ = nullptr;
    }
    reg_handle* h_ = nullptr;
    reg_pose_graph* g_ = nullptr;
};

// One submap collection (== one reg_submaps; o3d_slam::SubmapCollection) on the caller's handle, which must
// outlive it: every submap's map cloud, its occupancy keys and the overlap ring stay on the device; the switching state
// machine, the queues and the adjacency matrix live on the host inside the library.  Clouds are Open3D's fp64 arrays in host
// memory unless onDevice is set; transforms are column-major double[16]; stamps are nanoseconds.  The contract of every call
// is the header's text (include/o3dslam_reg.h).
class SubmapCollection {
public:
    struct Stamped { int32_t submapId; int64_t stampNs; };

    SubmapCollection(reg_handle* handle, const reg_submaps_params& params) : h_(handle), prm_(params) {
        const reg_status s = reg_submaps_create(h_, &params, &s_);
        if (s != REG_OK) raise(s, h_ ? reg_last_error(h_) : "no handle");
    }
    ~SubmapCollection() { if (s_) reg_submaps_destroy(s_); }   // before its handle
    SubmapCollection(const SubmapCollection&) = delete;
    SubmapCollection& operator=(const SubmapCollection&) = delete;

    void setMapToRangeSensor(const double T[16]) { check(reg_submaps_set_map_to_sensor(s_, T)); }
    // SubmapCollection::insertScan (SubmapCollection.cpp:189-245)
    reg_submaps_insert_result insertScan(const double* rawScan, int64_t nRaw, const double* points, const double* normals,
                                         const double* covariances, int64_t n, const double mapToRangeSensor[16], int64_t stampNs,
                                         bool onDevice = false) {
        reg_submaps_insert_result r{};
        r.struct_size = (int32_t)sizeof(r);
        check(reg_submaps_insert_scan(s_, rawScan, nRaw, points, normals, covariances, n, onDevice ? 1 : 0, mapToRangeSensor,
                                      stampNs, &r));
        return r;
    }
    reg_submaps_insert_result forceNewSubmapCreation() {
        reg_submaps_insert_result r{};
        r.struct_size = (int32_t)sizeof(r);
        check(reg_submaps_force_new_submap(s_, &r));
        return r;
    }
    // Submap::computeFeatures on the device from the resident map: the gate, the sparse cloud with its normals, its FPFH
    // features (n x 33) and the occupancy set; `ran` is false when the gate held (then nothing is handed out)
    struct Features {
        bool ran = false;
        std::vector<float> points, normals;
        std::vector<double> fpfh;
    };
    Features computeFeatures(int32_t submapId, double nowSeconds, const reg_submap_feature_params& params) {
        const size_t cap = (size_t)std::max<int64_t>(submapInfo(submapId).n_rows, 1);
        Features f;
        f.points.resize(cap * 3), f.normals.resize(cap * 3), f.fpfh.resize(cap * 33);
        int64_t n = 0;
        int32_t done = 0;
        check(reg_submaps_compute_features(s_, submapId, nowSeconds, &params, 0, f.points.data(), f.normals.data(), f.fpfh.data(),
                                           (int64_t)cap, &n, &done));
        f.ran = done != 0;
        f.points.resize((size_t)n * 3), f.normals.resize((size_t)n * 3), f.fpfh.resize((size_t)n * 33);
        return f;
    }
    // the gate and the occupancy set only; true when it ran
    bool computeFeatures(int32_t submapId, double nowSeconds) {
        int32_t done = 0;
        check(reg_submaps_compute_features(s_, submapId, nowSeconds, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &done));
        return done != 0;
    }
    bool isActiveSubmapEmpty() const { return submapInfo(info().active).n_rows == 0; }
    // cropSubmap + initReference of the active submap on handle(); returns the rows of the patch, 0 for an empty map or patch
    // (REG_EMPTY_TARGET: initReference returns false)
    int64_t setAsReference(const reg_crop* crop) {
        int64_t kept = 0;
        const reg_status st = reg_submaps_set_target(s_, crop, &kept);
        if (st == REG_EMPTY_TARGET) return 0;
        check(st);
        return kept;
    }
    void transform(const std::vector<int32_t>& ids, const std::vector<double>& dT) {
        if (dT.size() != ids.size() * 16) throw InvalidParameter("transform: dT must hold 16 doubles per id");
        check(reg_submaps_transform(s_, ids.data(), dT.data(), (int32_t)ids.size()));
    }
    void updateAdjacencyMatrix(const std::vector<int32_t>& source, const std::vector<int32_t>& target) {
        if (source.size() != target.size()) throw InvalidParameter("updateAdjacencyMatrix: one target per source");
        check(reg_submaps_add_loop_closure_edges(s_, source.data(), target.data(), (int32_t)source.size()));
    }
    std::vector<Stamped> popFinishedSubmapIds() { return pop(reg_submaps_pop_finished, info().n_finished); }
    std::vector<Stamped> popLoopClosureCandidates() {
        return pop(reg_submaps_pop_loop_closure_candidates, info().n_loop_closure_candidates);
    }
    void pushLoopClosureCandidate(int32_t submapId, int64_t stampNs) {
        check(reg_submaps_push_loop_closure_candidate(s_, submapId, stampNs));
    }
    std::vector<int32_t> getLoopClosureCandidatesIdxs(int32_t lastFinishedSubmapIdx) const {
        std::vector<int32_t> out((size_t)info().n_submaps);
        int32_t n = 0;
        check(reg_submaps_loop_closure_candidates(s_, lastFinishedSubmapIdx, out.data(), (int32_t)out.size(), &n));
        out.resize((size_t)n);
        return out;
    }
    // ---- every submap's dense map ----
    void enableDenseMaps(const reg_submaps_dense_params& params) { check(reg_submaps_enable_dense_maps(s_, &params)); }
    // Submap::insertScanDenseMap (Submap.cpp:98-113) of one submap: croppers, transform, insert, the carve when it is due
    reg_submaps_dense_insert_result insertScanDenseMap(int32_t submapId, const double* points, const double* normals,
                                                       const double* colors, int64_t n, const double mapToRangeSensor[16],
                                                       bool isPerformCarving = true, bool onDevice = false) {
        reg_submaps_dense_insert_result r{};
        r.struct_size = (int32_t)sizeof(r);
        check(reg_submaps_insert_scan_dense_map(s_, submapId, points, normals, colors, n, onDevice ? 1 : 0, mapToRangeSensor,
                                                isPerformCarving ? 1 : 0, &r));
        return r;
    }
    // getDenseMapCopy().toPointCloud() of one submap, in ascending key order
    DenseMap::Cloud exportDenseSubmap(int32_t submapId, bool wantKeys = false, bool wantCounts = false) {
        reg_dense_map_info i{};
        i.struct_size = (int32_t)sizeof(i);
        check(reg_submaps_get_dense_info(s_, submapId, &i, nullptr));
        const size_t rows = (size_t)i.n_voxels;
        DenseMap::Cloud out;
        out.points.resize(rows * 3);
        if (i.has_normals) out.normals.resize(rows * 3);
        if (i.has_colors) out.colors.resize(rows * 3);
        if (wantKeys) out.keys.resize(rows * 3);
        if (wantCounts) out.counts.resize(rows);
        int64_t k = 0;
        check(reg_submaps_export_dense_submap(s_, submapId, 0, out.points.data(), i.has_normals ? out.normals.data() : nullptr,
                                              i.has_colors ? out.colors.data() : nullptr, wantKeys ? out.keys.data() : nullptr,
                                              wantCounts ? out.counts.data() : nullptr, i.n_voxels, &k));
        return out;
    }
    // ---- pose-graph constraints from the resident maps ----
    struct Constraint {   // o3d_slam::Constraint
        int32_t sourceSubmapIdx = 0, targetSubmapIdx = 0;
        double sourceToTarget[16];      // column-major
        double informationMatrix[36];
        bool isInformationMatrixValid = false, isOdometryConstraint = false;
        int64_t timestampNs = 0;
    };
    reg_constraint_params odometryConstraintParams(bool refine = false) const {
        reg_constraint_params p{};
        check(reg_default_odometry_constraint_params(s_, refine ? 1 : 0, &p));
        return p;
    }
    // buildConstraint / the loop-closure refinement between two resident submaps; initial == nullptr: the identity
    reg_constraint_result buildConstraint(int32_t source, int32_t target, const reg_constraint_params& params,
                                          const double* initial = nullptr) {
        reg_constraint_result r{};
        r.struct_size = (int32_t)sizeof(r);
        check(reg_submaps_build_constraint(s_, source, target, &params, initial, &r));
        return r;
    }
    Constraint buildOdometryConstraint(int32_t source, int32_t target, bool refine = false) {
        return constraintOf(buildConstraint(source, target, odometryConstraintParams(refine)), true, 0);
    }
    // computeOdometryConstraints into the collection's own list: of the candidates, or (no argument) of every finished pair
    int32_t computeOdometryConstraints(const std::vector<int32_t>& candidates, bool refine = false) {
        if (candidates.empty()) return 0;
        const reg_constraint_params p = odometryConstraintParams(refine);
        int32_t added = 0;
        check(reg_submaps_compute_odometry_constraints(s_, candidates.data(), (int32_t)candidates.size(), &p, &added));
        return added;
    }
    int32_t computeOdometryConstraints(bool refine = false) {
        const reg_constraint_params p = odometryConstraintParams(refine);
        int32_t added = 0;
        check(reg_submaps_compute_odometry_constraints(s_, nullptr, 0, &p, &added));
        return added;
    }
    std::vector<Constraint> getOdometryConstraints() const {
        int32_t n = 0;
        check(reg_submaps_get_odometry_constraints(s_, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &n));
        std::vector<int32_t> src((size_t)std::max(n, 1)), tgt(src.size()), flags(src.size());
        std::vector<double> T(src.size() * 16), info(src.size() * 36);
        check(reg_submaps_get_odometry_constraints(s_, (int32_t)src.size(), src.data(), tgt.data(), T.data(), info.data(), flags.data(), &n));
        std::vector<Constraint> out((size_t)n);
        for (int32_t k = 0; k < n; ++k) {
            Constraint& c = out[(size_t)k];
            c.sourceSubmapIdx = src[(size_t)k], c.targetSubmapIdx = tgt[(size_t)k];
            std::copy(T.begin() + 16 * k, T.begin() + 16 * (k + 1), c.sourceToTarget);
            std::copy(info.begin() + 36 * k, info.begin() + 36 * (k + 1), c.informationMatrix);
            c.isInformationMatrixValid = (flags[(size_t)k] & 1) != 0, c.isOdometryConstraint = (flags[(size_t)k] & 2) != 0;
        }
        return out;
    }
    void clearOdometryConstraints() { check(reg_submaps_clear_odometry_constraints(s_)); }
    // buildLoopClosureConstraints of [(id, stamp)]: the accepted constraints; every verdict goes to *verdicts when given
    std::vector<Constraint> buildLoopClosureConstraints(const std::vector<Stamped>& candidates, const reg_loop_closure_params& params,
                                                        std::vector<reg_loop_closure_verdict>* verdicts = nullptr) {
        std::vector<Constraint> out;
        for (const Stamped& c : candidates) {
            std::vector<reg_loop_closure_verdict> v((size_t)std::max(info().n_submaps, 1));
            v[0].struct_size = (int32_t)sizeof(reg_loop_closure_verdict);
            int32_t n = 0;
            check(reg_submaps_build_loop_closure_constraints(s_, c.submapId, c.stampNs, &params, v.data(), (int32_t)v.size(), &n));
            for (int32_t k = 0; k < n; ++k) {
                if (verdicts) verdicts->push_back(v[(size_t)k]);
                if (v[(size_t)k].verdict == REG_LC_ACCEPTED) out.push_back(constraintOf(v[(size_t)k].constraint, false, c.stampNs));
            }
        }
        return out;
    }
    // Mapper::getAssembledMapPointCloud
    MapCloud::Cloud getAssembledMapPointCloud() {
        MapCloud::Cloud out;
        const int64_t rows = info().total_points;
        out.points.resize((size_t)rows * 3);
        if (prm_.map.has_normals) out.normals.resize((size_t)rows * 3);
        if (prm_.map.has_covariances) out.covariances.resize((size_t)rows * 9);
        int64_t k = 0;
        check(reg_submaps_export(s_, 0, out.points.data(), prm_.map.has_normals ? out.normals.data() : nullptr,
                                 prm_.map.has_covariances ? out.covariances.data() : nullptr, rows, &k));
        return out;
    }
    reg_submaps_info info() const {
        reg_submaps_info i{};
        i.struct_size = (int32_t)sizeof(i);
        check(reg_submaps_get_info(s_, &i));
        return i;
    }
    reg_submap_info submapInfo(int32_t idx) const {
        reg_submap_info i{};
        i.struct_size = (int32_t)sizeof(i);
        check(reg_submaps_get_submap_info(s_, idx, &i));
        return i;
    }
    reg_submaps* submaps() const { return s_; }
    reg_handle* handle() const { return h_; }

private:
    template <class F>
    std::vector<Stamped> pop(F fn, int32_t n) {
        std::vector<int32_t> ids((size_t)std::max(n, 1));
        std::vector<int64_t> stamps(ids.size());
        int32_t k = 0;
        check(fn(s_, ids.data(), stamps.data(), (int32_t)ids.size(), &k));
        std::vector<Stamped> out;
        for (int32_t i = 0; i < k; ++i) out.push_back(Stamped{ids[(size_t)i], stamps[(size_t)i]});
        return out;
    }
    static void raise(reg_status s, const std::string& msg) {
        if (s == REG_BAD_ARGUMENT) throw InvalidParameter(msg);
        if (s == REG_DEVICE_ERROR) throw DeviceError(msg);
        throw std::runtime_error(msg);
    }
    void check(reg_status s) const {
        if (s != REG_OK) raise(s, reg_last_error(h_));
    }
    static Constraint constraintOf(const reg_constraint_result& r, bool odometry, int64_t stampNs) {
        Constraint c;
        c.sourceSubmapIdx = r.source, c.targetSubmapIdx = r.target;
        std::copy(r.T, r.T + 16, c.sourceToTarget);
        std::copy(r.information, r.information + 36, c.informationMatrix);
        c.isInformationMatrixValid = r.information_estimated != 0, c.isOdometryConstraint = odometry;
        c.timestampNs = stampNs;
        return c;
    }
    reg_handle* h_ = nullptr;
    reg_submaps_params prm_;
    reg_submaps* s_ = nullptr;
};

// o3d_slam::TransformInterpolationBuffer as the Mapper uses it: (stamp, pose) pairs pushed in order (an earlier stamp is
// refused), capped at `limit`; lookup interpolates between the two neighbours (linear translation, slerp, factor =
// dt / (duration + 1e-6), Transform.cpp:16-67); getTransform clamps the time to the buffer.  Poses are column-major double[16].
class TransformBuffer {
public:
    explicit TransformBuffer(size_t limit = 2000) : limit_(limit) {}
    bool push(int64_t stampNs, const double T[16]) {
        if (!data_.empty() && stampNs < data_.back().stampNs) return false;
        StampedPose p;
        p.stampNs = stampNs;
        std::copy(T, T + 16, p.pose.begin());
        data_.push_back(p);
        if (data_.size() > limit_) data_.erase(data_.begin());
        return true;
    }
    bool empty() const { return data_.empty(); }
    size_t size() const { return data_.size(); }
    const std::vector<StampedPose>& entries() const { return data_; }
    int64_t earliestTime() const { need(); return data_.front().stampNs; }
    int64_t latestTime() const { need(); return data_.back().stampNs; }
    bool has(int64_t t) const { return !data_.empty() && earliestTime() <= t && t <= latestTime(); }
    std::array<double, 16> getTransform(int64_t t) const {   // o3d_slam::getTransform: clamped to the ends
        need();
        t = std::min(std::max(t, earliestTime()), latestTime());
        size_t k = 0;
        while (data_[k].stampNs < t) ++k;
        if (data_[k].stampNs == t || k == 0) return data_[k].pose;
        const StampedPose &a = data_[k - 1], &b = data_[k];
        const double f = ((double)(t - a.stampNs) * 1e-9) / ((double)(b.stampNs - a.stampNs) * 1e-9 + 1e-6);
        double qa[4], qb[4], q[4];
        quat(a.pose.data(), qa), quat(b.pose.data(), qb);
        double d = qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3], s0 = 1.0 - f, s1 = f;
        if (std::fabs(d) < 1.0 - std::numeric_limits<double>::epsilon()) {
            const double th = std::acos(std::fabs(d)), st = std::sin(th);
            s0 = std::sin((1.0 - f) * th) / st, s1 = std::sin(f * th) / st;
        }
        if (d < 0.0) s1 = -s1;
        for (int i = 0; i < 4; ++i) q[i] = s0 * qa[i] + s1 * qb[i];
        std::array<double, 16> T{};
        const double w = q[0], x = q[1], y = q[2], z = q[3], tx = 2 * x, ty = 2 * y, tz = 2 * z;
        T[0] = 1 - (ty * y + tz * z), T[4] = ty * x - tz * w, T[8] = tz * x + ty * w;
        T[1] = ty * x + tz * w, T[5] = 1 - (tx * x + tz * z), T[9] = tz * y - tx * w;
        T[2] = tz * x - ty * w, T[6] = tz * y + tx * w, T[10] = 1 - (tx * x + ty * y);
        for (int i = 0; i < 3; ++i) T[12 + i] = a.pose[12 + i] + (b.pose[12 + i] - a.pose[12 + i]) * f;
        T[15] = 1.0;
        return T;
    }

private:
    void need() const { if (data_.empty()) throw std::runtime_error("TransformInterpolationBuffer:: Empty buffer"); }
    static void quat(const double* T, double* q) {   // Eigen's Quaterniond(Matrix3d): (w, x, y, z); R(r, c) = T[4 c + r]
        auto R = [T](int r, int c) { return T[4 * c + r]; };
        double t = R(0, 0) + R(1, 1) + R(2, 2);
        if (t > 0.0) {
            t = std::sqrt(t + 1.0);
            q[0] = 0.5 * t, t = 0.5 / t;
            q[1] = (R(2, 1) - R(1, 2)) * t, q[2] = (R(0, 2) - R(2, 0)) * t, q[3] = (R(1, 0) - R(0, 1)) * t;
            return;
        }
        int i = R(1, 1) > R(0, 0) ? 1 : 0;
        if (R(2, 2) > R(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
        q[1 + i] = 0.5 * t, t = 0.5 / t;
        q[0] = (R(k, j) - R(j, k)) * t, q[1 + j] = (R(j, i) + R(i, j)) * t, q[1 + k] = (R(k, i) + R(i, k)) * t;
    }
    size_t limit_;
    std::vector<StampedPose> data_;
};

// o3d_slam::Mapper::addRangeMeasurement (Mapper.cpp:168-484) over one handle that carries the ICP configuration, a
// SubmapCollection on that handle and the odometry buffer (the Python mirror is icp.Mapper).  Per scan:
// reg_process_scan (the reading stays on the handle), reg_submaps_set_target when the reference is due, reg_register,
// reg_submaps_insert_scan.  Scans are host arrays (n x 3 doubles, sensor frame); stamps are nanoseconds; poses column-major.
// lastBranch() names the branch the last call ended in.  Departure: the map patch is cropped (and found empty) only when the
// reference is re-initialised.
struct MapperParameters {   // what addRangeMeasurement reads of o3d_slam::MapperParameters, Parameters.hpp:71,166,178-182
    bool isUseInitialMap = false, isMergeScansIntoMap = true;
    double mapMergeDelayInSeconds = 10.0, minMovementBetweenMappingSteps = 0.0, referenceCloudSettingPeriod = 1.0;
};
class Mapper {
public:
    using Parameters = MapperParameters;
    using Pose = std::array<double, 16>;

    Mapper(reg_handle* handle, SubmapCollection* submaps, const reg_scan_params& scan, const Parameters& params = Parameters())
        : h_(handle), submaps_(submaps), scan_(scan), params_(params) {
        cur_ = prev_ = lastInsertion_ = calibration_ = identity();
    }
    TransformBuffer& odometryBuffer() { return odom_; }
    const TransformBuffer& mapToRangeSensorBuffer() const { return poses_; }
    const TransformBuffer& bestGuessBuffer() const { return guesses_; }
    void setExternalOdometryFrameToCloudFrameCalibration(const double T[16]) { std::copy(T, T + 16, calibration_.begin()), calibrationSet_ = true; }
    void setMapToRangeSensor(const double T[16]) { std::copy(T, T + 16, cur_.begin()); }
    void setMapToRangeSensorInitial(const double T[16]) {
        if (newValueSet_) return;
        std::copy(T, T + 16, cur_.begin());
        prev_ = cur_, newValueSet_ = true;
    }
    const Pose& mapToRangeSensor() const { return cur_; }
    Pose getMapToRangeSensor(int64_t stampNs) const { return poses_.getTransform(stampNs); }
    MapCloud::Cloud getAssembledMapPointCloud() { return submaps_->getAssembledMapPointCloud(); }
    int referenceInitializations() const { return nReferenceInits_; }
    const std::string& lastBranch() const { return branch_; }

    bool addRangeMeasurement(const double* rawScan, int64_t n, int64_t stampNs) {
        if (!params_.isUseInitialMap && !calibrationSet_) return end("calibration_not_set", false);   // Mapper.cpp:169-174
        submaps_->setMapToRangeSensor(cur_.data());
        if (submaps_->isActiveSubmapEmpty()) {                                                          // :179-194
            if (params_.isUseInitialMap) {
                submaps_->insertScan(rawScan, n, rawScan, nullptr, nullptr, n, cur_.data(), stampNs);
                return end("first_scan_initial_map", true);
            }
            prev_ = cur_;
            const int64_t m = process(rawScan, n);
            submaps_->insertScan(rawScan, n, mergeXyz_.data(), mergeNrm(), nullptr, m, cur_.data(), stampNs);
            poses_.push(stampNs, cur_.data()), guesses_.push(stampNs, cur_.data());
            return end("first_scan", true);
        }
        if (stampNs <= lastStamp_) {                                                                    // :196-235
            const int64_t latest = odom_.latestTime();
            cur_ = guess(latest);
            poses_.push(latest, cur_.data()), guesses_.push(latest, prev_.data());
            submaps_->setMapToRangeSensor(cur_.data());
            prev_ = cur_;
            return end("out_of_order", true);
        }
        Pose estimate = prev_;
        if (odom_.has(stampNs) && !newValueSet_ && !ignoreOdometry_) estimate = guess(stampNs);        // :237-260
        ignoreOdometry_ = false;
        const int64_t m = process(rawScan, n);
        // :325-326: whole milliseconds, truncated (C++ division truncates towards zero); never initialised: always due
        const bool never = lastReferenceInit_ == std::numeric_limits<int64_t>::min();
        const double passed = never ? 0.0 : (double)((stampNs - lastReferenceInit_) / 1000000) / 1e3;
        if (newValueSet_ || never || passed >= params_.referenceCloudSettingPeriod) {                            // :329-347
            reg_crop crop = scan_.narrow;
            for (int k = 0; k < 3; ++k) crop.center[k] = cur_[12 + k];
            if (submaps_->setAsReference(&crop) == 0) return end("empty_map_patch", false);
            lastReferenceInit_ = stampNs;
            ++nReferenceInits_;
        }
        float Ti[16], To[16];
        for (int k = 0; k < 16; ++k) Ti[k] = To[k] = (float)estimate[k];
        reg_result res{};
        const reg_status st = reg_register(h_, Ti, To, &res);                                           // :372-373
        std::string branch = "registered";
        if (st == REG_DEVICE_ERROR || st == REG_BAD_ARGUMENT) throw std::runtime_error(reg_last_error(h_));
        if (st != REG_OK) {                                                                             // :400-402
            branch = "icp_exception";
            std::copy(Ti, Ti + 16, To);
        }
        if (newValueSet_) {                                                                             // :420-435
            initTime_ = stampNs, prev_ = cur_;
            poses_.push(stampNs, cur_.data()), guesses_.push(stampNs, estimate.data());
            newValueSet_ = false, ignoreOdometry_ = true;
            return end("new_value_set", true);
        }
        for (int k = 0; k < 16; ++k) cur_[k] = (double)To[k];                                           // :438-442
        poses_.push(stampNs, cur_.data()), guesses_.push(stampNs, estimate.data());
        submaps_->setMapToRangeSensor(cur_.data());
        const double sinceInit = (double)(stampNs - initTime_) * 1e-9;
        if (params_.isUseInitialMap && (!params_.isMergeScansIntoMap || sinceInit < params_.mapMergeDelayInSeconds)) {   // :445-459
            lastStamp_ = stampNs, prev_ = cur_;
            return end("merge_delay", true);
        }
        const double dx = cur_[12] - lastInsertion_[12], dy = cur_[13] - lastInsertion_[13], dz = cur_[14] - lastInsertion_[14];
        double mv[3];                                                                                   // :463-469: R_L^T (t_M - t_L)
        for (int i = 0; i < 3; ++i) mv[i] = (lastInsertion_[4 * i] * dx + lastInsertion_[4 * i + 1] * dy) + lastInsertion_[4 * i + 2] * dz;
        if (!(std::sqrt((mv[0] * mv[0] + mv[1] * mv[1]) + mv[2] * mv[2]) < params_.minMovementBetweenMappingSteps)) {
            lastInsert_ = submaps_->insertScan(rawScan, n, mergeXyz_.data(), mergeNrm(), nullptr, m, cur_.data(), stampNs);
            lastInsertion_ = cur_;
        } else {
            branch += "_moved_too_little";
        }
        lastStamp_ = stampNs, prev_ = cur_;
        return end(branch, true);
    }
    const reg_submaps_insert_result& lastInsert() const { return lastInsert_; }

private:
    static Pose identity() { return Pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; }
    bool end(const std::string& name, bool value) { branch_ = name; return value; }
    Pose guess(int64_t now) const {
        Pose out;
        const Pose a = odom_.getTransform(lastStamp_), b = odom_.getTransform(now);
        if (reg_host_mapper_initial_guess(prev_.data(), a.data(), b.data(), calibration_.data(), out.data()) != REG_OK)
            throw std::runtime_error("reg_host_mapper_initial_guess");
        return out;
    }
    const double* mergeNrm() const { return hasNormals_ ? mergeNrm_.data() : nullptr; }
    int64_t process(const double* raw, int64_t n) {   // processForScanMatchingAndMerging: match_ becomes the reading
        if (n <= 0) throw std::runtime_error("The reading point cloud is empty.");
        mergeXyz_.resize((size_t)n * 3), mergeNrm_.resize((size_t)n * 3);
        reg_scan_result r{};
        r.struct_size = (int32_t)sizeof(r);
        const reg_status st = reg_process_scan(h_, raw, nullptr, nullptr, n, 0, &scan_, mergeXyz_.data(), mergeNrm_.data(), nullptr, &r);
        if (st == REG_BAD_ARGUMENT) throw InvalidParameter(reg_last_error(h_));
        if (st != REG_OK) throw std::runtime_error(reg_last_error(h_));
        hasNormals_ = r.has_normals != 0;
        return r.n_merge;
    }
    reg_handle* h_;
    SubmapCollection* submaps_;
    reg_scan_params scan_;
    Parameters params_;
    TransformBuffer odom_, poses_, guesses_;
    Pose cur_, prev_, lastInsertion_, calibration_;
    bool calibrationSet_ = false, newValueSet_ = false, ignoreOdometry_ = false, hasNormals_ = false;
    int64_t lastStamp_ = std::numeric_limits<int64_t>::min(), lastReferenceInit_ = std::numeric_limits<int64_t>::min(), initTime_ = 0;
    int nReferenceInits_ = 0;
    std::string branch_;
    std::vector<double> mergeXyz_, mergeNrm_;
    reg_submaps_insert_result lastInsert_{};
};

}  // namespace o3dreg
