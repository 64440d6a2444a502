// Minimal C++ user of the drop-in mirror (include/o3dslam_icp.hpp): registers a noisy, displaced copy of a
// synthetic "two walls + floor" cloud against the original, the way o3d_slam::Mapper drives its icp_ member
// (initReference once, compute per scan).  Build: make -C examples ; run on an MI355X: ./examples/icp_demo
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../include/o3dslam_icp.hpp"

int main() {
    std::mt19937 rng(42);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    std::normal_distribution<float> noise(0.f, 0.005f);
    std::vector<float> ref, refn, rd, rdn;
    const int M = 60000, N = 8000;
    auto sample = [&](std::vector<float>& p, std::vector<float>& n) {
        const int f = (int)(u(rng) * 3.f);
        float x = 0, y = 0, z = 0, nx = 0, ny = 0, nz = 0;
        if (f == 0) { x = 10 * u(rng); y = 8 * u(rng); z = 0; nz = 1; }
        else if (f == 1) { x = 10 * u(rng); y = 0; z = 3 * u(rng); ny = 1; }
        else { x = 0; y = 8 * u(rng); z = 3 * u(rng); nx = 1; }
        p.insert(p.end(), {x + noise(rng), y + noise(rng), z + noise(rng), 1.f});
        n.insert(n.end(), {nx, ny, nz});
    };
    for (int i = 0; i < M; ++i) sample(ref, refn);
    for (int i = 0; i < N; ++i) sample(rd, rdn);
    // displace the reading by the inverse of (yaw 1 deg, t = (0.05, -0.03, 0.02))
    const float a = 1.0f * 3.14159265f / 180.f, c = std::cos(a), s = std::sin(a);
    for (int i = 0; i < N; ++i) {
        const float x = rd[4 * i] - 0.05f, y = rd[4 * i + 1] + 0.03f, z = rd[4 * i + 2] - 0.02f;
        rd[4 * i] = c * x + s * y;
        rd[4 * i + 1] = -s * x + c * y;
        rd[4 * i + 2] = z;
        const float nx = rdn[3 * i], ny = rdn[3 * i + 1];
        rdn[3 * i] = c * nx + s * ny;
        rdn[3 * i + 1] = -s * nx + c * ny;
    }
    try {
        o3dreg::ICP icp;
        icp.setShippedChain();
        o3dreg::DataPointsView reference{ref.data(), 4, M, refn.data(), 3};
        o3dreg::DataPointsView reading{rd.data(), 4, N, rdn.data(), 3};
        // SurfaceNormalDataPointsFilter on the device: the estimated reference normals must agree with the analytic
        // ones (up to sign) away from the wall/floor edges
        o3dreg::SurfaceNormalFilter sn;
        sn.knn = 10;
        sn.maxDist = 0.5f;
        std::vector<float> est(3 * (size_t)M);
        sn.compute(reference, est.data());
        int agree = 0;
        for (int i = 0; i < M; ++i) {
            const float d = est[3 * i] * refn[3 * i] + est[3 * i + 1] * refn[3 * i + 1] + est[3 * i + 2] * refn[3 * i + 2];
            if (std::fabs(d) > 0.95f) ++agree;
        }
        std::printf("estimated normals agree with the analytic ones on %.1f %% of the reference\n", 100.0 * agree / M);
        if (agree < 0.9 * M) return 4;
        if (!icp.initReference(reference)) return 2;
        const auto T = icp.compute(reading, reference, o3dreg::identity4(), false);
        const auto& r = icp.lastResult();
        std::printf("iterations %d converged %d inliers %lld  yaw %.4f deg  t = (%.4f, %.4f, %.4f)\n", r.iterations,
                    r.converged, (long long)r.n_inliers, std::atan2(T[1], T[0]) * 180.0 / 3.14159265, T[12], T[13], T[14]);
        const bool ok = std::fabs(std::atan2(T[1], T[0]) - a) < 2e-3 && std::fabs(T[12] - 0.05f) < 5e-3 &&
                        std::fabs(T[13] + 0.03f) < 5e-3 && std::fabs(T[14] - 0.02f) < 5e-3;
        // the same scan as Open3D holds it (fp64), cast on the device: the same transform
        std::vector<double> rd64(3 * (size_t)N), rdn64(3 * (size_t)N);
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < 3; ++k) {
                rd64[3 * i + k] = rd[4 * i + k];
                rdn64[3 * i + k] = rdn[3 * i + k];
            }
        const auto T64 = icp.computeF64(rd64.data(), rdn64.data(), N, false, o3dreg::identity4());
        bool same64 = true;
        for (int k = 0; k < 16; ++k) same64 = same64 && T64[k] == T[k];
        // the scan front end in one call with every stage switched off (no croppers, no voxel grid, ratio 1, the scan's
        // own normals): the merge cloud is the scan, the reading is the same fp32 cast, the transform the same again
        reg_scan_params sp;
        reg_default_scan_params(&sp);
        sp.wide.type = sp.narrow.type = REG_CROP_NONE;
        sp.voxel_size = 0.0;
        std::vector<double> merge(3 * (size_t)N), mergen(3 * (size_t)N);
        const reg_scan_result scan = icp.processScan(rd64.data(), rdn64.data(), nullptr, N, false, sp, merge.data(), mergen.data());
        const auto Ts = icp.registerPair(o3dreg::identity4());
        bool sameScan = scan.n_merge == N && scan.n_match == N && merge == rd64 && mergen == rdn64;
        for (int k = 0; k < 16; ++k) sameScan = sameScan && Ts[k] == T[k];
        std::printf("processScan (pass-through): %s\n", sameScan ? "identical" : "DIFFERENT");
        same64 = same64 && sameScan;
        // the multi-GPU loop (C++ steering + RCCL collectives) with a group of ONE rank: the same transform again
        icp.joinGroup(o3dreg::ICP::makeGroupId(), 0, 1);
        const auto Tp = icp.computePartitioned(reading, o3dreg::identity4());
        icp.leaveGroup();
        float dmax = 0.f;
        for (int k = 0; k < 16; ++k) dmax = std::fmax(dmax, std::fabs(Tp[k] - T[k]));
        std::printf("fp64 reading: %s; partitioned loop (1 rank, RCCL): max |dT| = %.2e\n", same64 ? "identical" : "DIFFERENT", dmax);
        // motion compensation of the fp64 scan on the device: zero velocities return it bit for bit, a moving sensor does not
        reg_params up;
        reg_default_params(&up);
        up.cost = REG_COST_O3D_P2P;
        reg_handle* uh = nullptr;
        if (reg_create(&up, &uh) != REG_OK) {
            reg_destroy(uh);
            return 5;
        }
        reg_undistort_params und{};
        und.struct_size = (int32_t)sizeof(und);
        und.spinning_clockwise = 1;
        und.scan_duration = 0.1;
        const bool still = o3dreg::undistortScan(uh, rd64.data(), N, und) == rd64;
        // the velocities from five poses 0.1 s apart, 0.1 m forward and 0.05 rad of yaw each: 1 m/s and 0.5 rad/s in the sensor frame
        std::vector<o3dreg::StampedPose> poses;
        for (int i = 0; i < 5; ++i) {
            o3dreg::StampedPose sp{(int64_t)i * 100000000, {}};
            const double yaw = 0.05 * i, cy = std::cos(yaw), sy = std::sin(yaw);
            sp.pose = {cy, sy, 0, 0, -sy, cy, 0, 0, 0, 0, 1, 0, 0.1 * i, 0, 0, 1};
            poses.push_back(sp);
        }
        o3dreg::estimateLinearAndAngularVelocity(poses, 500000000, 3, und.linear_velocity, und.angular_velocity_rpy);
        const bool velOk = std::fabs(und.angular_velocity_rpy[2] - 0.5) < 1e-4 && std::fabs(und.linear_velocity[0] - 1.0) < 0.02 &&
                           std::fabs(und.angular_velocity_rpy[0]) < 1e-12 && std::fabs(und.linear_velocity[2]) < 1e-12;
        const std::vector<double> moved = o3dreg::undistortScan(uh, rd64.data(), N, und);
        double far = 0.0;
        for (size_t k = 0; k < moved.size(); ++k) far = std::fmax(far, std::fabs(moved[k] - rd64[k]));
        reg_destroy(uh);
        const bool undOk = still && velOk && far > 0.01 && far < 1.0;
        std::printf("undistortScan: zero velocities %s, 1 m/s + 0.5 rad/s moves a point by at most %.3f m\n",
                    still ? "identical" : "DIFFERENT", far);
        // the resident LidarOdometry with the GICP operator on a scan that brings its normals: the first scan is kept, the
        // same scan again registers onto itself (identity, fitness 1) and the pose buffer gets one entry per scan
        reg_params gp;
        reg_default_params(&gp);
        gp.cost = REG_COST_GICP;
        gp.use_trimmed = 0;
        gp.gicp_stop_rule = 1;
        gp.max_dist = 0.5f;
        reg_odometry_params op;
        reg_default_odometry_params(&op);
        op.use_odometry_topic = 0;
        op.crop.type = REG_CROP_NONE;
        op.voxel_size = 0.0;
        op.normal_knn = 0;
        o3dreg::LidarOdometry odom(op, gp);
        const bool first = odom.addRangeScan(rd64.data(), rdn64.data(), N, 0);
        const bool second = odom.addRangeScan(rd64.data(), rdn64.data(), N, 100000000);
        const reg_odometry_result& orr = odom.lastResult();
        const bool odomOk = first && second && orr.registered && orr.fitness > 0.99 && std::fabs(orr.cumulative[12]) < 1e-4 &&
                            odom.getBuffer().size() == 2 && odom.getPreProcessedCloud().covariances.size() == 9 * (size_t)N &&
                            o3dreg::covariancesFromNormals(odom.handle(), rdn64.data(), N) == odom.getPreProcessedCloud().covariances;
        std::printf("LidarOdometry (GICP from normals): fitness %.3f, %d iterations, %s\n", orr.fitness, orr.iterations,
                    odomOk ? "consistent" : "INCONSISTENT");
        const bool ok2 = same64 && dmax < 1e-5f && undOk && odomOk;
        std::printf(ok && ok2 ? "OK\n" : "MISMATCH\n");
        return ok && ok2 ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
