// mapper_demo.cpp -- o3dreg::Mapper and o3dreg::SubmapCollection (include/o3dslam_icp.hpp) over a recorded walk: reads the
// scans, stamps and odometry poses that tests/test_gpu_mapper.py writes, runs Mapper::addRangeMeasurement on every scan and
// prints, per call, the branch, the active submap, the number of submaps and the pose as hexadecimal doubles, so that the
// test can compare them bit for bit with the Python mirror.  File (native endianness): int64 n_scans; double params[17]
// (radius, minNumRangeData, maxNumPoints, numScansOverlap, minFitness, maxSubmaps, mapVoxel, carveEvery, carveVoxel,
// mapCropRadius, matchCropRadius, scanVoxel, knn, knnRadius, referencePeriod, carvingEnabled, featureMask); double calib[16];
// double start[16]; per scan: int64 stamp, int64 pushOdometry, double odom[16], int64 n, double xyz[3 n].
// With a second argument `constraints` the odometry constraints of the finished pairs are built on the resident maps
// (SubmapCollection::computeOdometryConstraints) and printed before the final line.
#include "../include/o3dslam_icp.hpp"

#include <cstdio>
#include <memory>

template <class T>
static bool rd(FILE* f, T* out, size_t n) { return std::fread(out, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) return std::fprintf(stderr, "usage: mapper_demo WALK_FILE [constraints]\n"), 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    int64_t nScans = 0;
    double p[17], calib[16], start[16];
    if (!rd(f, &nScans, 1) || !rd(f, p, 17) || !rd(f, calib, 16) || !rd(f, start, 16)) return 2;

    reg_params rp;
    reg_shipped_params(&rp);
    reg_handle* h = nullptr;
    if (reg_create(&rp, &h) != REG_OK) return std::fprintf(stderr, "reg_create: %s\n", h ? reg_last_error(h) : "refused"), 3;
    int rc = 0;
    try {
        reg_submaps_params sp;
        reg_default_submaps_params(&sp);
        sp.radius = p[0], sp.min_num_range_data = (int32_t)p[1], sp.max_num_points = (int64_t)p[2];
        sp.num_scans_overlap = (int32_t)p[3], sp.revisit_min_fitness = p[4], sp.max_submaps = (int32_t)p[5];
        sp.map.map_voxel_size = p[6], sp.map.carve_every_n_scans = (int32_t)p[7], sp.map.carve_voxel_size = p[8];
        sp.map.crop.type = REG_CROP_MAX_RADIUS, sp.map.crop.radius_max = p[9], sp.is_carving_enabled = (int32_t)p[15];
        reg_scan_params scan;
        reg_default_scan_params(&scan);
        scan.wide = sp.map.crop;
        scan.narrow = sp.map.crop, scan.narrow.radius_max = p[10];
        scan.voxel_size = p[11], scan.down_sampling_ratio = 1.0, scan.seed = 0, scan.normal_knn = (int32_t)p[12], scan.normal_radius = p[13];
        o3dreg::SubmapCollection submaps(h, sp);
        o3dreg::Mapper::Parameters mp;
        mp.referenceCloudSettingPeriod = p[14];
        o3dreg::Mapper mapper(h, &submaps, scan, mp);
        mapper.setExternalOdometryFrameToCloudFrameCalibration(calib);
        mapper.setMapToRangeSensor(start);
        const int64_t featureMask = (int64_t)p[16];
        int64_t finished = 0;
        std::vector<double> xyz;
        for (int64_t k = 0; k < nScans; ++k) {
            int64_t stamp = 0, push = 0, n = 0;
            double odom[16];
            if (!rd(f, &stamp, 1) || !rd(f, &push, 1) || !rd(f, odom, 16) || !rd(f, &n, 1)) throw std::runtime_error("short file");
            xyz.resize((size_t)n * 3);
            if (!rd(f, xyz.data(), xyz.size())) throw std::runtime_error("short file");
            if (push) mapper.odometryBuffer().push(stamp, odom);
            const bool ok = mapper.addRangeMeasurement(xyz.data(), n, stamp);
            for (const auto& id : submaps.popFinishedSubmapIds()) {   // the feature thread's part: the occupancy set
                if ((featureMask >> finished) & 1) submaps.computeFeatures(id.submapId, 10.0 * (double)(finished + 1));
                ++finished;
            }
            const reg_submaps_info i = submaps.info();
            std::printf("%d %s %d %d %d", ok ? 1 : 0, mapper.lastBranch().c_str(), i.active, i.n_submaps, mapper.referenceInitializations());
            for (double v : mapper.mapToRangeSensor()) std::printf(" %a", v);
            std::printf("\n");
        }
        const auto cloud = mapper.getAssembledMapPointCloud();
        std::printf("MAP %lld %d\n", (long long)cloud.size(), (int)mapper.mapToRangeSensorBuffer().size());
        if (argc > 2 && std::string(argv[2]) == "constraints") {   // optional last step: the odometry constraints of the finished pairs
            const int32_t added = submaps.computeOdometryConstraints();
            std::printf("CONSTRAINTS %d\n", added);
            for (const auto& c : submaps.getOdometryConstraints()) {
                std::printf("ODOMETRY %d %d %d", c.sourceSubmapIdx, c.targetSubmapIdx, c.isInformationMatrixValid ? 1 : 0);
                for (double v : c.sourceToTarget) std::printf(" %a", v);
                for (double v : c.informationMatrix) std::printf(" %a", v);
                std::printf("\n");
            }
        }
        std::printf("OK\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mapper_demo: %s\n", e.what());
        rc = 1;
    }
    std::fclose(f);
    reg_destroy(h);
    return rc;
}
