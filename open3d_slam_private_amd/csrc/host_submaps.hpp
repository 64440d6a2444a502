// host_submaps.hpp -- the submap collection on the device: reg_submaps (o3d_slam::SubmapCollection with its
// AdjacencyMatrix, the candidate rule of PlaceRecognition and the pair selection of computeOdometryConstraints) over the map
// clouds of host_mapcloud.hpp, the occupancy sets of kernels_submaps.hpp and a ring of device copies of pre-processed scans;
// the pure host functions behind it (branch table, BFS, transform plan, the Mapper's initial guess).
// Part of the single translation unit reg_core.hip (included there, after host_posegraph.hpp; not a standalone header).
#pragma once

struct SmScan {   // one entry of overlapScansBuffer_ (ScanTimeTransform), resident
    DevBuf xyz, nrm, cov;
    int64_t n = 0, stamp = 0;
    double T[16];
};
struct SmSubmap {
    reg_map_cloud* map = nullptr;
    int32_t id = 0, parent = 0;
    bool center_computed = false, has_features = false;
    double origin[16], T_sensor[16], center[3] = {0, 0, 0}, feature_clock = 0.0;
    DevBuf keys[2];   // the occupancy set: built in the spare buffer, then swapped
    int cur = 0;
    int64_t n_keys = 0;
    DevBuf s_xyz64, s_xyz, s_nrm, s_fpfh;   // the feature store: sparseMapCloud_ (fp64, fp32), its normals, feature_
    int64_t n_sparse = 0;
    reg_dense_map* dense = nullptr;   // denseMap_: null until reg_submaps_enable_dense_maps
    int64_t dense_scans = 0;          // nScansInsertedDenseMap_
    ~SmSubmap() {
        reg_dense_map_destroy(dense);
        reg_map_cloud_destroy(map);
    }
};
struct SmConstraint {   // o3d_slam::Constraint
    int32_t source, target, flags;   // flags: bit 0 isInformationMatrixValid_, bit 1 isOdometryConstraint_
    double T[16], info[36];
};
struct SmStamped {
    int32_t id;
    int64_t stamp;
};
struct reg_submaps {
    reg_handle* h = nullptr;
    reg_submaps_params prm;
    std::vector<std::unique_ptr<SmSubmap>> subs;
    int32_t active = 0, scans_in_active = 0, last_finished = 0;
    bool force = false;
    double T_sensor[16];
    int64_t stamp = 0;
    std::unique_ptr<SmScan[]> slots;   // num_scans_overlap + 1: the spare one receives the next scan
    std::deque<int> ring;        // slot indices, oldest first
    std::vector<SmStamped> finished, candidates;
    std::vector<std::set<int32_t>> adj;   // AdjacencyMatrix::adjacency_
    std::vector<int32_t> marks;           // isLoopClosureSubmap_: -1 no entry, 0 false, 1 true
    DevBuf f_xyz64, f_xyz, f_nrm, f_fpfh; // the sparse cloud (fp64, fp32), its normals and FPFH of the last feature computation
    reg_handle* ch[4] = {nullptr, nullptr, nullptr, nullptr};   // the constraint builders' handles, by cost; created on first use
    std::vector<SmConstraint> odometry;   // odometryConstraints_
    DevBuf lc_ab, lc_ba, lc_cor, lc_inl;  // loop closure: nn_ab, nn_ba, the correspondences, RANSAC's inlier pairs
    bool dense_on = false;                // reg_submaps_enable_dense_maps has run
    reg_submaps_dense_params dprm;
    ~reg_submaps() {
        for (reg_handle* w : ch) reg_destroy(w);
    }
};

static void sm_add_edge(reg_submaps* s, int32_t a, int32_t b) {   // AdjacencyMatrix::addEdge: both marks become false
    s->adj[a].insert(b);
    s->adj[b].insert(a);
    s->marks[a] = s->marks[b] = 0;
}
static bool sm_adjacent(const reg_submaps* s, int32_t a, int32_t b) { return a == b || s->adj[a].count(b) != 0; }
static const double* sm_center(const SmSubmap& b) { return b.center_computed ? b.center : b.origin + 12; }
static double sm_dist(const double* a, const double* b) {   // (a - b).norm()
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
}
static void sm_mul(const double* A, const double* B, double* C) { pg_mul(B, A, C); }   // column-major A B (pg_mul is row-major)
static void sm_rigid_inverse(const double* T, double* O) {                              // column-major
    double r[16], ri[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r[4 * i + j] = T[4 * j + i];
    pg_rigid_inverse(r, ri);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) O[4 * j + i] = ri[4 * i + j];
}
static int sm_spare_slot(const reg_submaps* s) {
    for (int k = 0; k <= s->prm.num_scans_overlap; ++k)
        if (std::find(s->ring.begin(), s->ring.end(), k) == s->ring.end()) return k;
    return 0;   // not reached: the ring holds at most slots - 1 entries
}
static SmSubmap* sm_new_submap(reg_submaps* s, int32_t id, int32_t parent, const double* origin) {
    std::unique_ptr<SmSubmap> b(new SmSubmap());
    if (reg_map_cloud_create(s->h, &s->prm.map, &b->map) != REG_OK) return nullptr;
    if (s->dense_on && reg_dense_map_create(s->h, s->dprm.voxel_size, &b->dense) != REG_OK) return nullptr;
    b->id = id;
    b->parent = parent;
    std::memcpy(b->origin, origin, sizeof(b->origin));
    od_identity(b->T_sensor);
    return b.release();
}

// The occupancy set of submap b from its current map cloud, into the spare key buffer; swapped in at the end.
static reg_status sm_build_keys(reg_submaps* s, SmSubmap& b) {
    reg_handle* h = s->h;
    const int64_t n = b.map->n;
    if (n == 0) {
        b.n_keys = 0;
        return REG_OK;
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, h->dm.reserve((size_t)n));
    const RunArrays a = h->dm.arrays();
    const double inv = 1.0 / (s->prm.voxel_expansion_factor * s->prm.map.map_voxel_size);
    k_occ_keys<<<grid_for(n), 256, 0, h->stream>>>(mc_cur(b.map).xyz, n, inv, a.keys, a.vals);
    uint32_t tail[2];
    uint64_t first = 0;
    REGCHK(sort_runs(h, a, n, tail));
    HIPCHK(h, hipMemcpyAsync(&first, a.sorted, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    const int64_t n_keys = flag_total(tail) - (first == kOccNoKey ? 1 : 0);
    DevBuf& out = b.keys[b.cur ^ 1];
    HIPCHK(h, dm_grow(out, (size_t)std::max<int64_t>(n_keys, 1), 8));
    if (n_keys > 0) {
        k_occ_unique<<<grid_for(n), 256, 0, h->stream>>>(a.sorted, n, a.heads, a.run, out.as<uint64_t>());
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
    }
    b.cur ^= 1;
    b.n_keys = n_keys;
    return REG_OK;
}

// isSwitchingSubmapsConsistant's count and fitness of n device points at pose T against the set of b
static reg_status sm_fitness(reg_submaps* s, const SmSubmap& b, const double* d_xyz, int64_t n, const double* T, int64_t* count,
                             double* fitness) {
    reg_handle* h = s->h;
    uint32_t c = 0;
    if (n > 0 && b.n_keys > 0) {
        HIPCHK(h, hipSetDevice(h->prm.device));
        HIPCHK(h, h->dm_misc.reserve(256));
        uint32_t* d_c = (uint32_t*)((char*)h->dm_misc.p + 128);
        HIPCHK(h, hipMemsetAsync(d_c, 0, 4, h->stream));
        const double inv = 1.0 / (s->prm.voxel_expansion_factor * s->prm.map.map_voxel_size);
        k_occ_count<<<grid_for(n), 256, 0, h->stream>>>(d_xyz, n, xform_rows(T), inv, b.keys[b.cur].as<uint64_t>(), b.n_keys, d_c);
        HIPCHK(h, hipMemcpyAsync(&c, d_c, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
    }
    *count = (int64_t)c;
    *fitness = n > 0 ? (double)c / (double)n : std::numeric_limits<double>::quiet_NaN();   // 0 / 0 of the reference
    return REG_OK;
}

// Submap::insertScan of a resident scan (device pointers) into submap b
static reg_status sm_insert(reg_submaps* s, SmSubmap& b, const double* d_raw, int64_t n_raw, SmScan& sc, bool carve,
                            reg_map_cloud_insert_result* res) {
    if (sc.n == 0) return REG_OK;   // Submap.cpp:41-43
    const bool nrm = s->prm.map.has_normals, cov = s->prm.map.has_covariances;
    const double *x = sc.xyz.as<double>(), *nr = nrm ? sc.nrm.as<double>() : nullptr, *cv = cov ? sc.cov.as<double>() : nullptr;
    if (s->prm.is_use_initial_map && b.map->n == 0)   // Submap.cpp:47-52
        return reg_map_cloud_set(b.map, x, nr, cv, sc.n, 1, s->prm.map.map_voxel_size);
    return reg_map_cloud_insert_scan(b.map, d_raw, n_raw, x, nr, cv, sc.n, 1, sc.T, carve && s->prm.is_carving_enabled, res);
}

static bool sm_idx_ok(const reg_submaps* s, int32_t idx) { return idx >= 0 && idx < (int32_t)s->subs.size(); }

extern "C" {

void reg_default_submaps_params(reg_submaps_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_submaps_params);
    p->max_submaps = 64;
    p->num_scans_overlap = 3;     // SubmapParameters, Parameters.hpp:103-110
    p->min_num_range_data = 5;
    p->is_carving_enabled = 0;   // MapperParameters::isCarvingEnabled_, Parameters.hpp:181
    p->min_submaps_between_loop_closures = 2;   // PlaceRecognitionParameters, Parameters.hpp:138-139
    p->max_num_points = 400000;
    p->radius = 20.0;
    p->revisit_min_fitness = 0.4;
    p->voxel_expansion_factor = 2.5;   // magic.hpp:16
    p->min_seconds_between_features = 5.0;
    p->loop_closure_search_radius = 20.0;
    reg_default_map_cloud_params(&p->map);
}

reg_status reg_check_submaps_params(const reg_submaps_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(reg_submaps_params)) return REG_BAD_ARGUMENT;
    const double v = p->voxel_expansion_factor * p->map.map_voxel_size;
    if (p->max_submaps < 1 || p->max_submaps > 4096 || p->num_scans_overlap < 1 || p->max_num_points < 0 ||
        p->radius != p->radius || p->revisit_min_fitness != p->revisit_min_fitness || !(v > 0.0) || !std::isfinite(v) ||
        !std::isfinite(1.0 / v) || p->min_seconds_between_features != p->min_seconds_between_features ||
        p->loop_closure_search_radius != p->loop_closure_search_radius || p->map.struct_size != (int32_t)sizeof(reg_map_cloud_params))
        return REG_BAD_ARGUMENT;
    return REG_OK;
}

void reg_submaps_struct_sizes(int32_t sizes[5]) {
    if (!sizes) return;
    sizes[0] = (int32_t)sizeof(reg_submaps_params);
    sizes[1] = (int32_t)sizeof(reg_submaps_info);
    sizes[2] = (int32_t)sizeof(reg_submap_info);
    sizes[3] = (int32_t)sizeof(reg_submaps_insert_result);
    sizes[4] = (int32_t)sizeof(reg_submap_feature_params);
}

int32_t reg_host_submaps_decide(int32_t force_flag, int32_t scans_in_active, int32_t min_num_range_data, int32_t is_use_initial_map,
                                int64_t active_points, int64_t max_num_points, int32_t closest_is_active,
                                double distance_to_closest, double distance_to_active, double radius, int32_t adjacent,
                                int32_t fitness_ok) {
    if (force_flag) return REG_SUBMAPS_CREATE | REG_SUBMAPS_FORCED;        // SubmapCollection.cpp:95-99
    if (scans_in_active < min_num_range_data) return REG_SUBMAPS_KEEP;     // :101-103
    if (is_use_initial_map) return REG_SUBMAPS_KEEP;                       // :105-107
    const int32_t flag = active_points > max_num_points ? REG_SUBMAPS_SET_FORCE_FLAG : 0;   // :114-116
    if (!(distance_to_closest < radius)) return REG_SUBMAPS_CREATE | flag;                  // :122, :144-147
    if (closest_is_active) return REG_SUBMAPS_KEEP | flag;                                  // :127-129
    if (adjacent) {                                                                         // :132-135
        if (fitness_ok < 0) return REG_SUBMAPS_NEED_FITNESS | flag;
        if (fitness_ok) return REG_SUBMAPS_SWITCH | flag;
    }
    return (distance_to_active > radius ? REG_SUBMAPS_CREATE : REG_SUBMAPS_KEEP) | flag;    // :138-142
}

int32_t reg_host_adjacency_distance(const uint8_t* adj, const int32_t* marks, int32_t n, int32_t id) {
    if (!adj || !marks || n < 1 || id < 0 || id >= n) return -1;
    bool any = false;
    for (int32_t i = 0; i < n; ++i) any = any || marks[i] >= 0;
    if (!any) return std::numeric_limits<int32_t>::max();   // AdjacencyMatrix.cpp:24-26
    std::vector<int32_t> parent(n, -1), queue;
    std::vector<char> visited(n, 0);
    visited[id] = 1;
    queue.push_back(id);
    int32_t v = id;
    for (size_t head = 0; head < queue.size(); ++head) {
        v = queue[head];
        if (marks[v] < 0) return -1;   // isLoopClosureSubmap_.at(v) / adjacency_.at(v) throw
        if (marks[v] > 0) break;
        for (int32_t a = 0; a < n; ++a)   // std::set: ascending
            if (adj[(size_t)v * n + a] && !visited[a]) {
                visited[a] = 1;
                queue.push_back(a);
                parent[a] = v;
            }
    }
    int32_t distance = 0;
    while (v != id) {
        v = parent[v];
        ++distance;
    }
    return std::max(0, distance - 1);
}

reg_status reg_host_submaps_transform_plan(const int32_t* parents, int32_t n_submaps, const int32_t* ids, int32_t n, int32_t* plan) {
    if (!parents || !plan || n_submaps < 1 || n < 0 || (n > 0 && !ids)) return REG_BAD_ARGUMENT;
    for (int32_t i = 0; i < n_submaps; ++i) {
        plan[i] = -1;
        if (parents[i] < 0 || parents[i] >= n_submaps) return REG_BAD_ARGUMENT;
    }
    std::vector<char> listed(n_submaps, 0);
    for (int32_t k = 0; k < n; ++k)
        if (ids[k] >= 0 && ids[k] < n_submaps) listed[ids[k]] = 1, plan[ids[k]] = k;   // SubmapCollection.cpp:328-338
    if (n == 0) return REG_OK;   // `while (true && !transformIncrements.empty())`
    for (int32_t idx = 0; idx < n_submaps; ++idx) {
        if (listed[idx]) continue;
        int32_t cur = idx;
        for (;;) {   // :356-368
            cur = parents[cur];
            if (listed[cur]) {
                if (cur >= n) return REG_BAD_TRANSFORM;   // transformIncrements.at(currentNode): a POSITION, reproduced
                plan[idx] = cur;
                break;
            }
            if (cur == parents[cur]) return REG_BAD_TRANSFORM;   // "Stuck in a loop, this should not happen"
        }
    }
    return REG_OK;
}

reg_status reg_host_mapper_initial_guess(const double prev_map_to_sensor[16], const double odom_prev[16], const double odom_now[16],
                                         const double calib[16], double out[16]) {
    if (!prev_map_to_sensor || !odom_prev || !odom_now || !calib || !out) return REG_BAD_ARGUMENT;
    double ci[16], a[16], b[16], bi[16], m[16], r[16];
    sm_rigid_inverse(calib, ci);
    sm_mul(odom_now, ci, a);
    sm_mul(odom_prev, ci, b);
    sm_rigid_inverse(b, bi);
    sm_mul(bi, a, m);
    sm_mul(prev_map_to_sensor, m, r);
    std::memcpy(out, r, sizeof(r));
    return REG_OK;
}

reg_status reg_submaps_create(reg_handle* h, const reg_submaps_params* p, reg_submaps** out) {
    if (!h || !out) return REG_BAD_ARGUMENT;
    *out = nullptr;
    if (reg_check_submaps_params(p) != REG_OK) {
        h->err = "reg_submaps_create: params missing or of the wrong struct_size (map's included), max_submaps outside [1, 4096], "
                 "num_scans_overlap < 1, max_num_points < 0, a NaN, or voxel_expansion_factor * map.map_voxel_size not finite and > 0";
        return REG_BAD_ARGUMENT;
    }
    std::unique_ptr<reg_submaps> s(new reg_submaps());
    s->h = h;
    s->prm = *p;
    od_identity(s->T_sensor);
    SmSubmap* first = sm_new_submap(s.get(), 0, 0, s->T_sensor);   // SubmapCollection.cpp:28-32
    if (!first) return REG_BAD_ARGUMENT;                           // the map cloud's own refusal; its text is in h->err
    s->subs.emplace_back(first);
    s->slots.reset(new SmScan[(size_t)p->num_scans_overlap + 1]);
    s->adj.resize((size_t)p->max_submaps);
    s->marks.assign((size_t)p->max_submaps, -1);
    *out = s.release();
    return REG_OK;
}

void reg_submaps_destroy(reg_submaps* s) {
    if (!s) return;
    if (s->h->device_ok && hipSetDevice(s->h->prm.device) == hipSuccess) (void)hipStreamSynchronize(s->h->stream);
    delete s;
}

reg_status reg_submaps_get_info(const reg_submaps* s, reg_submaps_info* info) {
    if (!s || !info || info->struct_size != (int32_t)sizeof(reg_submaps_info)) return REG_BAD_ARGUMENT;
    info->n_submaps = (int32_t)s->subs.size();
    info->active = s->active;
    info->force_new_submap = s->force;
    info->scans_in_active = s->scans_in_active;
    info->ring_size = (int32_t)s->ring.size();
    info->n_finished = (int32_t)s->finished.size();
    info->n_loop_closure_candidates = (int32_t)s->candidates.size();
    info->last_finished = s->last_finished;
    info->reserved = 0;
    info->total_points = 0;
    for (const auto& b : s->subs) info->total_points += b->map->n;
    info->stamp_ns = s->stamp;
    std::memcpy(info->T_map_to_sensor, s->T_sensor, sizeof(s->T_sensor));
    return REG_OK;
}

reg_status reg_submaps_get_submap_info(const reg_submaps* s, int32_t idx, reg_submap_info* info) {
    if (!s || !info || info->struct_size != (int32_t)sizeof(reg_submap_info) || !sm_idx_ok(s, idx)) return REG_BAD_ARGUMENT;
    const SmSubmap& b = *s->subs[idx];
    info->id = b.id;
    info->parent = b.parent;
    info->center_computed = b.center_computed;
    info->features_computed = b.has_features;
    info->reserved = 0;
    info->n_rows = b.map->n;
    info->scans_inserted = b.map->scans;
    info->n_keys = b.n_keys;
    std::memcpy(info->origin, b.origin, sizeof(b.origin));
    std::memcpy(info->T_map_to_sensor, b.T_sensor, sizeof(b.T_sensor));
    for (int k = 0; k < 3; ++k) info->center[k] = sm_center(b)[k], info->crop_center[k] = b.map->center[k];
    info->feature_clock = b.feature_clock;
    return REG_OK;
}

reg_status reg_submaps_set_map_to_sensor(reg_submaps* s, const double T[16]) {
    if (!s || !T) return REG_BAD_ARGUMENT;
    std::memcpy(s->T_sensor, T, sizeof(s->T_sensor));
    return REG_OK;
}

reg_status reg_submaps_insert_scan(reg_submaps* s, const double* raw_xyz, int64_t n_raw, const double* scan_xyz,
                                   const double* scan_normals, const double* scan_covs, int64_t n, int on_device,
                                   const double T[16], int64_t stamp_ns, reg_submaps_insert_result* res) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    const int32_t prev = s->active;
    SmSubmap& act = *s->subs[prev];
    if (res && res->struct_size != (int32_t)sizeof(reg_submaps_insert_result)) {
        h->err = "reg_submaps_insert_scan: result of the wrong struct_size";
        return REG_BAD_ARGUMENT;
    }
    if (!T || !mc_cloud_ok(act.map, scan_xyz, scan_normals, scan_covs, n) || !dm_cloud_args_ok(raw_xyz, n_raw)) {
        h->err = std::string("reg_submaps_insert_scan: T missing, a bad raw scan, or a scan not") + kMcCloudMsg;
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));

    // 1. the scan into the spare slot of the ring (SubmapCollection.cpp:206); it joins the ring when the call commits
    const int slot = sm_spare_slot(s);
    SmScan& sc = s->slots[slot];
    const double* src[3] = {scan_xyz, scan_normals, scan_covs};
    DevBuf* dst[3] = {&sc.xyz, &sc.nrm, &sc.cov};
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (int k = 0; k < 3; ++k)
        if (n > 0 && src[k]) {
            HIPCHK(h, dm_grow(*dst[k], (size_t)n, kSpWidth[k] * 8));
            HIPCHK(h, hipMemcpyAsync(dst[k]->p, src[k], (size_t)n * kSpWidth[k] * 8, kind, h->stream));
        }
    sc.n = n;
    sc.stamp = stamp_ns;
    std::memcpy(sc.T, T, sizeof(sc.T));
    // the raw scan is staged only when the carve of the receiving map is due (the rule of reg_map_cloud_insert_scan)
    const bool carve_due = s->prm.is_carving_enabled && act.map->n > 0 && (act.map->scans % act.map->prm.carve_every_n_scans) == 1 &&
                           !(s->prm.is_use_initial_map && act.map->n == 0);
    const double* d_raw = nullptr;
    if (n > 0 && n_raw > 0 && carve_due) HIPCHK(h, staged_input(h, h->mc_in[3], raw_xyz, (size_t)n_raw * 3, on_device, &d_raw));
    if (!d_raw) n_raw = 0;

    // 2. updateActiveSubmap (:94-148) on the state as it stands
    int32_t closest = 0;
    for (int32_t i = 1; i < (int32_t)s->subs.size(); ++i)   // findClosestSubmap: std::min_element, the first minimum
        if (sm_dist(T + 12, sm_center(*s->subs[i])) < sm_dist(T + 12, sm_center(*s->subs[closest]))) closest = i;
    const double d_closest = sm_dist(T + 12, sm_center(*s->subs[closest])), d_active = sm_dist(T + 12, sm_center(act));
    const int32_t adjacent = sm_adjacent(s, s->subs[closest]->id, act.id);
    int32_t fitness_ok = -1, dec;
    int64_t count = 0;
    double fitness = 0.0;
    for (;;) {
        dec = reg_host_submaps_decide(s->force, s->scans_in_active, s->prm.min_num_range_data, s->prm.is_use_initial_map,
                                      act.map->n, s->prm.max_num_points, closest == prev, d_closest, d_active, s->prm.radius,
                                      adjacent, fitness_ok);
        if ((dec & REG_SUBMAPS_ACTION_MASK) != REG_SUBMAPS_NEED_FITNESS) break;
        REGCHK(sm_fitness(s, *s->subs[closest], sc.xyz.as<double>(), n, T, &count, &fitness));
        fitness_ok = fitness > s->prm.revisit_min_fitness ? 1 : 0;   // a NaN fails
    }
    const int action = dec & REG_SUBMAPS_ACTION_MASK;
    std::unique_ptr<SmSubmap> created;
    int32_t now = prev;
    if (action == REG_SUBMAPS_SWITCH) now = closest;
    if (action == REG_SUBMAPS_CREATE) {   // createNewSubmap (:150-162)
        now = (int32_t)s->subs.size();
        if (now >= s->prm.max_submaps) {
            h->err = "reg_submaps_insert_scan: a new submap is due and max_submaps is exhausted";
            return REG_BAD_ARGUMENT;
        }
        created.reset(sm_new_submap(s, now, prev, T));
        if (!created) return REG_BAD_ARGUMENT;
    }

    // 3. the device steps
    reg_map_cloud_insert_result ins;
    std::memset(&ins, 0, sizeof(ins));
    ins.struct_size = (int32_t)sizeof(ins);
    ins.n_rows = act.map->n;
    REGCHK(sm_insert(s, act, d_raw, n_raw, sc, true, &ins));   // :214 / :238: the previous active submap either way
    double center[3] = {0, 0, 0};
    int32_t drained = 0;
    int last_filled = -1;
    if (now != prev) {
        REGCHK(reg_map_cloud_center(act.map, center));   // computeSubmapCenter (:217)
        SmSubmap& target = created ? *created : *s->subs[now];
        std::deque<int> order = s->ring;                 // the ring as the push leaves it
        order.push_back(slot);
        if ((int)order.size() > s->prm.num_scans_overlap) order.pop_front();
        for (int k : order) {                            // insertBufferedScans (:87-92)
            SmScan& b = s->slots[k];
            REGCHK(sm_insert(s, target, b.xyz.as<double>(), b.n, b, false, nullptr));
            if (b.n > 0) last_filled = k;
            ++drained;
        }
    }

    // 4. commit the host state
    std::memcpy(s->T_sensor, T, sizeof(s->T_sensor));
    s->stamp = stamp_ns;
    if (n > 0) std::memcpy(act.T_sensor, T, sizeof(act.T_sensor));   // Submap.cpp:45
    if (dec & REG_SUBMAPS_FORCED) s->force = false;
    if (dec & REG_SUBMAPS_SET_FORCE_FLAG) s->force = true;
    if (now != prev) {
        for (int k = 0; k < 3; ++k) act.center[k] = center[k];
        act.center_computed = true;
        if (created) s->subs.emplace_back(created.release());
        SmSubmap& target = *s->subs[now];
        if (last_filled >= 0) std::memcpy(target.T_sensor, s->slots[last_filled].T, sizeof(target.T_sensor));
        s->active = now;
        s->last_finished = prev;
        s->finished.push_back(SmStamped{prev, stamp_ns});
        s->scans_in_active = 0;
        sm_add_edge(s, act.id, target.id);
        s->ring.clear();
    } else {
        s->ring.push_back(slot);
        if ((int)s->ring.size() > s->prm.num_scans_overlap) s->ring.pop_front();
    }
    s->scans_in_active += 1;
    if (res) {   // written only by a call that succeeds
        std::memset(res, 0, sizeof(*res));
        res->struct_size = (int32_t)sizeof(*res);
        res->previous_active = prev;
        res->decision = dec;
        res->active = now;
        res->fitness_computed = fitness_ok >= 0;
        res->ring_drained = drained;
        res->fitness_count = count;
        res->fitness = fitness;
        res->insert = ins;
    }
    return REG_OK;
}

reg_status reg_submaps_force_new_submap(reg_submaps* s, reg_submaps_insert_result* res) {
    if (!s) return REG_BAD_ARGUMENT;
    const bool before = s->force;
    s->force = true;   // SubmapCollection.cpp:184-186
    const double T[16] = {s->T_sensor[0],  s->T_sensor[1],  s->T_sensor[2],  s->T_sensor[3], s->T_sensor[4],  s->T_sensor[5],
                          s->T_sensor[6],  s->T_sensor[7],  s->T_sensor[8],  s->T_sensor[9], s->T_sensor[10], s->T_sensor[11],
                          s->T_sensor[12], s->T_sensor[13], s->T_sensor[14], s->T_sensor[15]};
    const reg_status st = reg_submaps_insert_scan(s, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, T, s->stamp, res);
    s->force = st == REG_OK ? false : before;
    return st;
}

void reg_default_submap_feature_params(reg_submap_feature_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(*p);
    p->normal_knn = 10;   // PlaceRecognitionParameters, Parameters.hpp:121-126
    p->feature_knn = 100;
    p->feature_voxel_size = 0.5;
    p->normal_radius = 1.0;
    p->feature_radius = 2.5;
}

// The sparse cloud and its FPFH features of submap b into the collection's feature buffers: what reg_voxel_down_sample,
// reg_estimate_normals and reg_compute_fpfh do, called with device pointers on the collection's handle.
static reg_status sm_features(reg_submaps* s, SmSubmap& b, const reg_submap_feature_params* fp, int64_t* n_sparse) {
    reg_handle* h = s->h;
    const int64_t n = b.map->n;
    *n_sparse = 0;
    if (n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, dm_grow(s->f_xyz64, (size_t)n, 24));
    int64_t m = 0;
    REGCHK(reg_voxel_down_sample(h, mc_cur(b.map).xyz, nullptr, nullptr, n, 1, fp->feature_voxel_size, s->f_xyz64.as<double>(), nullptr,
                                 nullptr, &m));
    HIPCHK(h, dm_grow(s->f_xyz, (size_t)m, 12));
    HIPCHK(h, dm_grow(s->f_nrm, (size_t)m, 12));
    HIPCHK(h, dm_grow(s->f_fpfh, (size_t)m, 33 * 8));
    k_cast_cloud_f64<<<grid_for(m), 256, 0, h->stream>>>(s->f_xyz64.as<double>(), nullptr, nullptr, m, s->f_xyz.as<float>(), nullptr,
                                                         nullptr);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    reg_normals_out no;
    std::memset(&no, 0, sizeof(no));
    no.normals = s->f_nrm.as<float>();
    const float origin[3] = {0.f, 0.f, 0.f};   // OrientNormalsTowardsCameraLocation(Zero), Submap.cpp:271
    REGCHK(reg_estimate_normals(h, s->f_xyz.as<float>(), 3, m, 1, fp->normal_knn, (float)fp->normal_radius, origin, 0, &no, nullptr));
    REGCHK(reg_compute_fpfh(h, s->f_xyz.as<float>(), 3, s->f_nrm.as<float>(), 3, m, 1, fp->feature_knn, (float)fp->feature_radius,
                            s->f_fpfh.as<double>(), nullptr, nullptr, nullptr));
    *n_sparse = m;
    return REG_OK;
}

// The feature store of submap b: m rows of the collection's feature buffers, device to device, on the stream.
// The rows count only once every copy is queued: a failure here leaves the submap without stored features.
static reg_status sm_store_features(reg_submaps* s, SmSubmap& b, int64_t m) {
    reg_handle* h = s->h;
    b.n_sparse = 0;
    if (m == 0) return REG_OK;
    DevBuf* dst[4] = {&b.s_xyz64, &b.s_xyz, &b.s_nrm, &b.s_fpfh};
    const DevBuf* src[4] = {&s->f_xyz64, &s->f_xyz, &s->f_nrm, &s->f_fpfh};
    const size_t row[4] = {24, 12, 12, 33 * 8};
    for (int k = 0; k < 4; ++k) {
        HIPCHK(h, dst[k]->reserve((size_t)m * row[k]));
        HIPCHK(h, hipMemcpyAsync(dst[k]->p, src[k]->p, (size_t)m * row[k], hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    b.n_sparse = m;
    return REG_OK;
}

reg_status reg_submaps_compute_features(reg_submaps* s, int32_t idx, double now_seconds, const reg_submap_feature_params* fp,
                                        int on_device, float* sparse_xyz, float* sparse_normals, double* fpfh,
                                        int64_t capacity_rows, int64_t* n_sparse, int32_t* computed) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    if (computed) *computed = 0;
    if (n_sparse) *n_sparse = 0;
    if (!sm_idx_ok(s, idx) || now_seconds != now_seconds ||
        (fp && (fp->struct_size != (int32_t)sizeof(*fp) || !(fp->feature_voxel_size > 0.0) || !std::isfinite(fp->feature_voxel_size) ||
                fp->normal_knn < 1 || fp->normal_knn > kPcaMaxK || !(fp->normal_radius > 0.0) || fp->feature_knn < 2 ||
                fp->feature_knn > kFpfhMaxNn || !(fp->feature_radius > 0.0) || !std::isfinite(fp->feature_radius) || capacity_rows < 0))) {
        h->err = "reg_submaps_compute_features: an unknown submap index, a NaN clock, or feature params of the wrong struct_size, "
                 "voxel size / radii not finite and > 0, normal_knn outside [1, 32], feature_knn outside [2, 128], capacity_rows < 0";
        return REG_BAD_ARGUMENT;
    }
    SmSubmap& b = *s->subs[idx];
    if (b.has_features && now_seconds - b.feature_clock < s->prm.min_seconds_between_features) return REG_OK;   // Submap.cpp:256-258
    if (!h->device_ok) return REG_DEVICE_ERROR;
    int64_t m = 0;
    if (fp) {   // sparseMapCloud_ and feature_ (Submap.cpp:266-272)
        REGCHK(sm_features(s, b, fp, &m));
        if (m > capacity_rows) {
            h->err = "reg_submaps_compute_features: capacity_rows is below the rows of the sparse cloud";
            return REG_BAD_ARGUMENT;
        }
    }
    REGCHK(sm_build_keys(s, b));   // voxelMap_.clear(); voxelMap_.insertCloud(...)
    if (m > 0) {
        HIPCHK(h, copy_out(h, sparse_xyz, s->f_xyz.p, (size_t)m * 12, on_device));
        HIPCHK(h, copy_out(h, sparse_normals, s->f_nrm.p, (size_t)m * 12, on_device));
        HIPCHK(h, copy_out(h, fpfh, s->f_fpfh.p, (size_t)m * 33 * 8, on_device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (fp) REGCHK(sm_store_features(s, b, m));
    b.has_features = true;
    b.feature_clock = now_seconds;   // featureTimer_.reset()
    if (n_sparse) *n_sparse = m;
    if (computed) *computed = 1;
    return REG_OK;
}

reg_status reg_submaps_get_keys(reg_submaps* s, int32_t idx, uint64_t* keys, int64_t capacity_rows, int64_t* n_out) {
    if (!s) return REG_BAD_ARGUMENT;
    if (n_out) *n_out = 0;
    if (!sm_idx_ok(s, idx) || (keys && capacity_rows < s->subs[idx]->n_keys)) {
        s->h->err = "reg_submaps_get_keys: an unknown submap index, or capacity_rows below the number of keys";
        return REG_BAD_ARGUMENT;
    }
    const SmSubmap& b = *s->subs[idx];
    if (n_out) *n_out = b.n_keys;
    if (!keys || b.n_keys == 0) return REG_OK;
    reg_handle* h = s->h;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, hipMemcpyAsync(keys, b.keys[b.cur].p, (size_t)b.n_keys * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

reg_status reg_submaps_switch_fitness(reg_submaps* s, int32_t idx, const double* scan_xyz, int64_t n, int on_device,
                                      const double T[16], int64_t* count, double* fitness) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    if (!sm_idx_ok(s, idx) || !T || !dm_cloud_args_ok(scan_xyz, n)) {
        h->err = "reg_submaps_switch_fitness: an unknown submap index, T missing, or not 0 <= n <= 2^31 - 1 with points for n > 0";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d = scan_xyz;
    if (n > 0) HIPCHK(h, staged_input(h, h->mc_in[0], d, (size_t)n * 3, on_device, &d));
    int64_t c = 0;
    double f = 0.0;
    REGCHK(sm_fitness(s, *s->subs[idx], d, n, T, &c, &f));
    if (count) *count = c;
    if (fitness) *fitness = f;
    return REG_OK;
}

reg_status reg_submaps_set_target(reg_submaps* s, const reg_crop* crop, int64_t* n_kept) {
    if (!s) return REG_BAD_ARGUMENT;
    return reg_map_cloud_set_target(s->subs[s->active]->map, crop, n_kept);
}

reg_status reg_submaps_export_submap(reg_submaps* s, int32_t idx, int on_device, double* xyz, double* normals, double* covs,
                                     int64_t capacity_rows, int64_t* n_out) {
    if (!s) return REG_BAD_ARGUMENT;
    if (n_out) *n_out = 0;
    if (!sm_idx_ok(s, idx)) {
        s->h->err = "reg_submaps_export_submap: an unknown submap index";
        return REG_BAD_ARGUMENT;
    }
    return reg_map_cloud_export(s->subs[idx]->map, on_device, xyz, normals, covs, capacity_rows, n_out);
}

reg_status reg_submaps_export(reg_submaps* s, int on_device, double* xyz, double* normals, double* covs, int64_t capacity_rows,
                              int64_t* n_out) {
    if (!s) return REG_BAD_ARGUMENT;
    if (n_out) *n_out = 0;
    int64_t total = 0;
    for (const auto& b : s->subs) total += b->map->n;
    if (capacity_rows < total) {
        s->h->err = "reg_submaps_export: capacity_rows is below the number of rows";
        return REG_BAD_ARGUMENT;
    }
    int64_t off = 0;
    for (const auto& b : s->subs) {
        int64_t k = 0;
        REGCHK(reg_map_cloud_export(b->map, on_device, xyz ? xyz + 3 * off : nullptr, normals ? normals + 3 * off : nullptr,
                                    covs ? covs + 9 * off : nullptr, capacity_rows - off, &k));
        off += k;
    }
    if (n_out) *n_out = off;
    return REG_OK;
}

reg_status reg_submaps_transform(reg_submaps* s, const int32_t* ids, const double* dT, int32_t n) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    const int32_t ns = (int32_t)s->subs.size();
    if (n < 0 || (n > 0 && (!ids || !dT))) {
        h->err = "reg_submaps_transform: n < 0, or ids / dT missing";
        return REG_BAD_ARGUMENT;
    }
    std::vector<int32_t> parents(ns), plan(ns);
    for (int32_t i = 0; i < ns; ++i) parents[i] = s->subs[i]->parent;
    const reg_status st = reg_host_submaps_transform_plan(parents.data(), ns, ids, n, plan.data());
    if (st != REG_OK) {
        h->err = "reg_submaps_transform: stuck in a loop (an unlisted submap whose parent chain ends at an unlisted root), or a "
                 "parent index beyond the list of increments";
        return st;
    }
    auto apply = [&](SmSubmap& b, const double* T) -> reg_status {   // Submap::transform (Submap.cpp:115-128)
        REGCHK(reg_map_cloud_transform(b.map, T));
        if (b.dense) REGCHK(reg_dense_map_transform(b.dense, T));   // denseMap_.transform (Submap.cpp:122-125)
        if (b.n_sparse > 0) {   // sparseMapCloud_.Transform (Submap.cpp:117); feature_ stays
            HIPCHK(h, hipSetDevice(h->prm.device));
            k_sm_transform_sparse<<<grid_for(b.n_sparse), 256, 0, h->stream>>>(b.s_xyz64.as<double>(), b.s_xyz.as<float>(),
                                                                              b.s_nrm.as<float>(), b.n_sparse, xform_rows(T));
            HIPCHK(h, hipGetLastError());
        }
        double m[16], c[3];
        sm_mul(b.T_sensor, T, m);
        std::memcpy(b.T_sensor, m, sizeof(m));
        for (int r = 0; r < 3; ++r) {
            double v = T[r] * b.center[0] + T[4 + r] * b.center[1];
            v = v + T[8 + r] * b.center[2];
            c[r] = v + T[12 + r];
        }
        for (int r = 0; r < 3; ++r) b.center[r] = c[r];
        return REG_OK;
    };
    for (int32_t k = 0; k < n; ++k)   // the listed ones, in list order
        if (ids[k] >= 0 && ids[k] < ns) REGCHK(apply(*s->subs[ids[k]], dT + 16 * (size_t)k));
    std::vector<char> listed(ns, 0);
    for (int32_t k = 0; k < n; ++k)
        if (ids[k] >= 0 && ids[k] < ns) listed[ids[k]] = 1;
    for (int32_t i = 0; i < ns; ++i)
        if (!listed[i] && plan[i] >= 0) REGCHK(apply(*s->subs[i], dT + 16 * (size_t)plan[i]));
    s->ring.clear();   // :372
    return REG_OK;
}

// ---- the dense maps of the collection ----
void reg_default_submaps_dense_params(reg_submaps_dense_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_submaps_dense_params);
    p->carve_every_n_scans = 10;   // SpaceCarvingParameters, Parameters.hpp:88-95
    p->voxel_size = 0.03;          // MapBuilderParameters::mapVoxelSize_
    reg_default_dense_scan_params(&p->scan);
    reg_default_dense_carve_params(&p->carve);
}

reg_status reg_check_submaps_dense_params(const reg_submaps_dense_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(reg_submaps_dense_params)) return REG_BAD_ARGUMENT;
    CropCfg crop;
    DmOffsets off;
    if (p->carve_every_n_scans < 1 || (p->carve_in_map_frame != 0 && p->carve_in_map_frame != 1) || !(p->voxel_size > 0.0) ||
        !std::isfinite(p->voxel_size) || !dm_scan_params_ok(&p->scan, &crop) || !dm_carve_params_ok(&p->carve, p->voxel_size, &off))
        return REG_BAD_ARGUMENT;
    return REG_OK;
}

void reg_submaps_dense_struct_sizes(int32_t sizes[2]) {
    if (!sizes) return;
    sizes[0] = (int32_t)sizeof(reg_submaps_dense_params);
    sizes[1] = (int32_t)sizeof(reg_submaps_dense_insert_result);
}

reg_status reg_submaps_enable_dense_maps(reg_submaps* s, const reg_submaps_dense_params* p) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    if (s->dense_on) {
        h->err = "reg_submaps_enable_dense_maps: the collection has dense maps already";
        return REG_BAD_ARGUMENT;
    }
    if (reg_check_submaps_dense_params(p) != REG_OK) {
        h->err = "reg_submaps_enable_dense_maps: params missing or of a wrong struct_size (scan's and carve's included), "
                 "carve_every_n_scans < 1, carve_in_map_frame not 0 / 1, voxel_size not finite and > 0, an unknown crop type, a "
                 "NaN colour bound, or carve parameters reg_dense_map_carve refuses at this voxel size";
        return REG_BAD_ARGUMENT;
    }
    std::vector<reg_dense_map*> made;   // holds no device memory until the first insert: all or nothing
    for (size_t k = 0; k < s->subs.size(); ++k) {
        reg_dense_map* m = nullptr;
        if (reg_dense_map_create(h, p->voxel_size, &m) != REG_OK) {
            for (reg_dense_map* d : made) reg_dense_map_destroy(d);
            return REG_BAD_ARGUMENT;
        }
        made.push_back(m);
    }
    for (size_t k = 0; k < s->subs.size(); ++k) s->subs[k]->dense = made[k];
    s->dprm = *p;
    s->dense_on = true;
    return REG_OK;
}

reg_status reg_submaps_insert_scan_dense_map(reg_submaps* s, int32_t idx, const double* xyz, const double* normals,
                                             const double* colors, int64_t n, int on_device, const double T[16],
                                             int32_t perform_carving, reg_submaps_dense_insert_result* res) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    if (!s->dense_on) {
        h->err = "reg_submaps_insert_scan_dense_map: dense maps are not enabled (reg_submaps_enable_dense_maps)";
        return REG_NOT_CONFIGURED;
    }
    if (!sm_idx_ok(s, idx) || !T || !dm_cloud_args_ok(xyz, n) || (res && res->struct_size != (int32_t)sizeof(*res))) {
        h->err = "reg_submaps_insert_scan_dense_map: an unknown submap, T missing, a bad scan (0 <= n <= 2^31 - 1 and a cloud for "
                 "n > 0), or a result of the wrong struct_size";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    SmSubmap& b = *s->subs[idx];
    HIPCHK(h, hipSetDevice(h->prm.device));
    // the scan is uploaded once: both steps read the device copy
    const double* d[3] = {xyz, normals, colors};
    if (n > 0)
        for (int k = 0; k < 3; ++k) HIPCHK(h, staged_input(h, h->dm_in[k], d[k], (size_t)n * 3, on_device, &d[k]));
    int64_t n_inserted = 0, n_voxels = b.dense->n, n_removed = 0;
    REGCHK(reg_dense_map_insert_scan(b.dense, d[0], d[1], d[2], n, 1, &s->dprm.scan, T, &n_inserted, &n_voxels));   // Submap.cpp:99-106
    const bool carve = perform_carving && b.dense->n > 0 && b.dense_scans % s->dprm.carve_every_n_scans == 1;   // :146-149
    if (carve && n > 0) {
        DmOffsets off;
        dm_offsets(s->dprm.carve.neighborhood_radius, b.dense->voxel, &off);   // checked when the maps were enabled
        REGCHK(dm_carve_scan_device(b.dense, "reg_submaps_insert_scan_dense_map", d[0], n, T + 12, &s->dprm.carve, off,
                                    s->dprm.carve_in_map_frame ? T : nullptr, 1, nullptr, &n_removed));
    }
    b.dense_scans += 1;   // :111
    if (res) {
        std::memset(res, 0, sizeof(*res));
        res->struct_size = (int32_t)sizeof(*res);
        res->carved = carve;
        res->n_inserted = n_inserted;
        res->n_voxels = b.dense->n;
        res->n_removed = n_removed;
        res->scans_inserted = b.dense_scans;
    }
    return REG_OK;
}

reg_status reg_submaps_get_dense_info(const reg_submaps* s, int32_t idx, reg_dense_map_info* info, int64_t* scans_inserted) {
    if (!s) return REG_BAD_ARGUMENT;
    if (!s->dense_on) {
        s->h->err = "reg_submaps_get_dense_info: dense maps are not enabled (reg_submaps_enable_dense_maps)";
        return REG_NOT_CONFIGURED;
    }
    if (!sm_idx_ok(s, idx)) return REG_BAD_ARGUMENT;
    if (info) REGCHK(reg_dense_map_get_info(s->subs[idx]->dense, info));
    if (scans_inserted) *scans_inserted = s->subs[idx]->dense_scans;
    return REG_OK;
}

reg_status reg_submaps_export_dense_submap(reg_submaps* s, int32_t idx, int on_device, double* xyz, double* normals, double* colors,
                                           int32_t* keys, int32_t* counts, int64_t capacity_rows, int64_t* n_out) {
    if (!s) return REG_BAD_ARGUMENT;
    if (n_out) *n_out = 0;
    if (!s->dense_on) {
        s->h->err = "reg_submaps_export_dense_submap: dense maps are not enabled (reg_submaps_enable_dense_maps)";
        return REG_NOT_CONFIGURED;
    }
    if (!sm_idx_ok(s, idx)) {
        s->h->err = "reg_submaps_export_dense_submap: an unknown submap";
        return REG_BAD_ARGUMENT;
    }
    return reg_dense_map_export(s->subs[idx]->dense, on_device, xyz, normals, colors, keys, counts, capacity_rows, n_out);
}

reg_status reg_submaps_add_loop_closure_edges(reg_submaps* s, const int32_t* source, const int32_t* target, int32_t n) {
    if (!s) return REG_BAD_ARGUMENT;
    bool ok = n >= 0 && (n == 0 || (source && target));
    for (int32_t k = 0; ok && k < n; ++k) ok = sm_idx_ok(s, source[k]) && sm_idx_ok(s, target[k]);
    if (!ok) {
        s->h->err = "reg_submaps_add_loop_closure_edges: n < 0, arrays missing, or an unknown submap id";
        return REG_BAD_ARGUMENT;
    }
    for (int32_t k = 0; k < n; ++k) {   // SubmapCollection.cpp:75-81
        sm_add_edge(s, source[k], target[k]);
        s->marks[source[k]] = s->marks[target[k]] = 1;
    }
    return REG_OK;
}

reg_status reg_submaps_get_adjacency(const reg_submaps* s, uint8_t* adj, int32_t* marks, int32_t capacity) {
    if (!s || capacity < (int32_t)s->subs.size()) return REG_BAD_ARGUMENT;
    if (adj) std::memset(adj, 0, (size_t)capacity * capacity);
    for (int32_t i = 0; i < capacity; ++i) {
        const bool known = i < (int32_t)s->subs.size();
        if (marks) marks[i] = known ? s->marks[i] : -1;
        if (adj && known)
            for (int32_t j : s->adj[i]) adj[(size_t)i * capacity + j] = 1;
    }
    return REG_OK;
}

static reg_status sm_pop(reg_submaps* s, std::vector<SmStamped>& q, int32_t* ids, int64_t* stamps, int32_t capacity, int32_t* n_out) {
    if (n_out) *n_out = 0;
    if (capacity < (int32_t)q.size() || (!q.empty() && !ids)) {
        s->h->err = "reg_submaps_pop_*: capacity below the entries of the queue, or ids missing";
        return REG_BAD_ARGUMENT;
    }
    for (size_t k = 0; k < q.size(); ++k) {
        ids[k] = q[k].id;
        if (stamps) stamps[k] = q[k].stamp;
    }
    if (n_out) *n_out = (int32_t)q.size();
    q.clear();
    return REG_OK;
}
reg_status reg_submaps_pop_finished(reg_submaps* s, int32_t* ids, int64_t* stamps_ns, int32_t capacity, int32_t* n_out) {
    return s ? sm_pop(s, s->finished, ids, stamps_ns, capacity, n_out) : REG_BAD_ARGUMENT;
}
reg_status reg_submaps_pop_loop_closure_candidates(reg_submaps* s, int32_t* ids, int64_t* stamps_ns, int32_t capacity,
                                                   int32_t* n_out) {
    return s ? sm_pop(s, s->candidates, ids, stamps_ns, capacity, n_out) : REG_BAD_ARGUMENT;
}
reg_status reg_submaps_push_loop_closure_candidate(reg_submaps* s, int32_t id, int64_t stamp_ns) {
    if (!s || !sm_idx_ok(s, id)) return REG_BAD_ARGUMENT;
    s->candidates.push_back(SmStamped{id, stamp_ns});
    return REG_OK;
}

reg_status reg_submaps_loop_closure_candidates(const reg_submaps* s, int32_t last, int32_t* out, int32_t capacity, int32_t* n_out) {
    if (!s || !n_out || !sm_idx_ok(s, last) || capacity < 0 || (capacity > 0 && !out)) return REG_BAD_ARGUMENT;
    *n_out = 0;
    const int32_t ns = (int32_t)s->subs.size();
    std::vector<uint8_t> adj((size_t)ns * ns);
    std::vector<int32_t> marks(ns);
    (void)reg_submaps_get_adjacency(s, adj.data(), marks.data(), ns);
    const double max_d = s->prm.loop_closure_search_radius;
    const int threshold = (int)std::ceil(max_d / s->prm.radius);
    std::vector<int32_t> found;
    for (int32_t i = 0; i < ns; ++i) {   // PlaceRecognition.cpp:239-282
        if (i == s->active) continue;
        if (sm_adjacent(s, s->subs[i]->id, s->subs[s->active]->id)) continue;
        if (std::abs(i - last) == 1 || sm_adjacent(s, i, last)) continue;
        if (sm_dist(sm_center(*s->subs[last]), sm_center(*s->subs[i])) > max_d) continue;
        if (std::abs(i - last) <= threshold) continue;
        const int32_t d = reg_host_adjacency_distance(adj.data(), marks.data(), ns, last);
        if (d < 0) return REG_BAD_ARGUMENT;   // the reference would throw: last_finished has no entry in the matrix
        if (d < s->prm.min_submaps_between_loop_closures) continue;
        found.push_back(i);
    }
    if ((int32_t)found.size() > capacity) return REG_BAD_ARGUMENT;
    for (size_t k = 0; k < found.size(); ++k) out[k] = found[k];
    *n_out = (int32_t)found.size();
    return REG_OK;
}

reg_status reg_submaps_odometry_constraint_pairs(const reg_submaps* s, const int32_t* candidates, int32_t n_candidates,
                                                 const int32_t* existing, int32_t n_existing, int32_t* out, int32_t capacity,
                                                 int32_t* n_out) {
    if (!s || !n_out || n_candidates < 0 || n_existing < 0 || (n_existing > 0 && !existing) || capacity < 0 || (capacity > 0 && !out))
        return REG_BAD_ARGUMENT;
    *n_out = 0;
    for (int32_t k = 0; candidates && k < n_candidates; ++k)
        if (!sm_idx_ok(s, candidates[k])) return REG_BAD_ARGUMENT;
    std::vector<int32_t> pairs;
    auto has = [&](int32_t a, int32_t b) {   // hasConstraint
        for (int32_t k = 0; k < n_existing; ++k)
            if (existing[2 * k] == a && existing[2 * k + 1] == b) return true;
        for (size_t k = 0; k + 1 < pairs.size(); k += 2)
            if (pairs[k] == a && pairs[k + 1] == b) return true;
        return false;
    };
    const int32_t active = s->subs[s->active]->id, count = candidates ? n_candidates : (int32_t)s->subs.size() - 1;
    for (int32_t k = 0; k < count; ++k) {
        const int32_t tgt = candidates ? candidates[k] : k + 1;
        if (tgt < 1) continue;   // constraint_builders.cpp:96-98
        const int32_t src = s->subs[tgt]->parent;
        if (has(src, tgt)) continue;
        if (!candidates && (src == active || tgt == active)) continue;   // :113
        pairs.push_back(src);
        pairs.push_back(tgt);
    }
    if ((int32_t)(pairs.size() / 2) > capacity) return REG_BAD_ARGUMENT;
    for (size_t k = 0; k < pairs.size(); ++k) out[k] = pairs[k];
    *n_out = (int32_t)(pairs.size() / 2);
    return REG_OK;
}

}  // extern "C"

// ---- pose-graph constraints from the resident collection ---------------------------------------------------------
static const char* kSmConstraintMsg =
    ": params missing or of the wrong struct_size, a cost other than REG_COST_O3D_P2PL / REG_COST_O3D_P2P / REG_COST_GICP, "
    "max_iteration < 1, icp_max_correspondence_distance not finite and > 0, information_max_distance not in "
    "(0, icp_max_correspondence_distance], or an overlap voxel not finite and > 0";

// The builders' handle for `cost`: created on first use with the parameters of the stateless operators (reg_default_params,
// the cost, no trimming, Open3D's stop rule for GICP), on the collection's stream -- as normals_workspace does it.
static reg_status sm_constraint_handle(reg_submaps* s, int32_t cost, reg_handle** out) {
    reg_handle* h = s->h;
    if (!s->ch[cost]) {
        reg_params p;
        reg_default_params(&p);
        p.cost = cost;
        p.use_trimmed = 0;
        p.max_dist = 1.f;   // set per call
        p.device = h->prm.device;
        if (cost == REG_COST_GICP) p.gicp_stop_rule = 1;
        reg_handle* w = nullptr;
        const reg_status cs = reg_create(&p, &w);
        if (cs != REG_OK) {
            h->err = std::string("reg_submaps_build_constraint: handle: ") + reg_last_error(w);
            reg_destroy(w);
            return cs;
        }
        s->ch[cost] = w;
    }
    const reg_status ss = reg_set_stream(s->ch[cost], h->stream);
    if (ss != REG_OK) {
        h->err = s->ch[cost]->err;
        return ss;
    }
    *out = s->ch[cost];
    return REG_OK;
}

extern "C" {

void reg_constraints_struct_sizes(int32_t sizes[2]) {
    if (!sizes) return;
    sizes[0] = (int32_t)sizeof(reg_constraint_params);
    sizes[1] = (int32_t)sizeof(reg_constraint_result);
}

reg_status reg_check_constraint_params(const reg_constraint_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(reg_constraint_params)) return REG_BAD_ARGUMENT;
    if (p->cost != REG_COST_O3D_P2PL && p->cost != REG_COST_O3D_P2P && p->cost != REG_COST_GICP) return REG_BAD_ARGUMENT;
    if (p->max_iteration < 1 || !std::isfinite(p->icp_max_correspondence_distance) || !(p->icp_max_correspondence_distance > 0.0) ||
        !(p->information_max_distance > 0.0) || !(p->information_max_distance <= p->icp_max_correspondence_distance) ||
        !((float)p->icp_max_correspondence_distance > 0.f) || !std::isfinite((float)p->icp_max_correspondence_distance))
        return REG_BAD_ARGUMENT;
    if (p->is_compute_overlap && (!std::isfinite(p->overlap_voxel_size) || !(p->overlap_voxel_size > 0.0))) return REG_BAD_ARGUMENT;
    return REG_OK;
}

reg_status reg_default_odometry_constraint_params(const reg_submaps* s, int refine, reg_constraint_params* p) {
    if (!s || !p) return REG_BAD_ARGUMENT;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(*p);
    // getMapVoxelSize(mapBuilder_, magic::voxelSizeCorrespondenceSearchIfMapVoxelSizeIsZero), constraint_builders.cpp:34-38,
    // helpers.cpp:356-358: "zero" is |voxel| <= 1e-3
    const double voxel = std::fabs(s->prm.map.map_voxel_size) <= 1e-3 ? 0.04 : s->prm.map.map_voxel_size;
    p->cost = REG_COST_O3D_P2PL;
    p->max_iteration = 100;   // magic::icpRunUntilConvergenceNumberOfIterations
    p->is_compute_overlap = 1;
    p->skip_refinement = refine ? 0 : 1;
    p->estimate_information = 1;
    p->overlap_voxel_size = 20.0 * voxel;                 // magic::voxelExpansionFactorOverlapComputation
    p->icp_max_correspondence_distance = 1.5 * voxel;     // magic::voxelExpansionFactorIcpCorrespondenceDistance
    p->information_max_distance = p->icp_max_correspondence_distance;
    return REG_OK;
}

reg_status reg_submaps_build_constraint(reg_submaps* s, int32_t source, int32_t target, const reg_constraint_params* p,
                                        const double T_init[16], reg_constraint_result* out) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    if (reg_check_constraint_params(p) != REG_OK || !out || out->struct_size != (int32_t)sizeof(reg_constraint_result)) {
        h->err = std::string("reg_submaps_build_constraint: result missing or of the wrong struct_size, or") + (kSmConstraintMsg + 1);
        return REG_BAD_ARGUMENT;
    }
    if (!sm_idx_ok(s, source) || !sm_idx_ok(s, target) || source == target) {
        h->err = "reg_submaps_build_constraint: an unknown submap index, or source == target";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    reg_handle* w = nullptr;
    REGCHK(sm_constraint_handle(s, p->cost, &w));
    reg_map_cloud *ms = s->subs[source]->map, *mt = s->subs[target]->map;
    const Cols64 cs = mc_cur(ms), ct = mc_cur(mt);
    const bool gicp = p->cost == REG_COST_GICP;
    const double* t_nrm = p->cost == REG_COST_O3D_P2PL ? ct.nrm : nullptr;
    const double *s_cov = gicp ? cs.aux : nullptr, *t_cov = gicp ? ct.aux : nullptr;
    w->prm.max_dist = (float)p->icp_max_correspondence_distance;
    w->prm.max_iter = p->max_iteration;
    auto fail = [&](reg_status st) {
        h->err = std::string("reg_submaps_build_constraint: ") + w->err;
        return st;
    };
    reg_constraint_result r;
    std::memset(&r, 0, sizeof(r));
    r.struct_size = (int32_t)sizeof(r);
    r.source = source;
    r.target = target;
    reg_status st;
    if (p->is_compute_overlap) {
        st = reg_set_pair_overlap_f64(w, ms->n > 0 ? cs.xyz : nullptr, nullptr, s_cov, ms->n, mt->n > 0 ? ct.xyz : nullptr, t_nrm, t_cov,
                                      mt->n, 1, T_init, p->overlap_voxel_size, 1, &r.n_source_selected, &r.n_target_selected);
        if (st != REG_OK) return fail(st);
    } else {
        st = reg_set_target_f64(w, ct.xyz, t_nrm, t_cov, mt->n, 1, nullptr, &r.n_target_selected);
        if (st != REG_OK) return fail(st);
        st = reg_set_source_f64(w, cs.xyz, nullptr, s_cov, ms->n, 1);
        if (st != REG_OK) return fail(st);
        r.n_source_selected = ms->n;
    }
    float Ti[16], To[16];
    for (int k = 0; k < 16; ++k) Ti[k] = T_init ? (float)T_init[k] : (k % 5 == 0 ? 1.f : 0.f);
    std::memcpy(To, Ti, sizeof(To));
    if (!p->skip_refinement) {
        reg_result res;
        std::memset(&res, 0, sizeof(res));
        st = reg_register(w, Ti, To, &res);
        if (st != REG_OK) return fail(st);
        r.refined = 1;
        r.iterations = res.iterations;
        r.converged = res.converged;
        r.fitness = res.fitness;
        r.inlier_rmse = res.inlier_rmse;
    }
    for (int k = 0; k < 16; ++k) r.T[k] = (double)To[k];
    for (int k = 0; k < 36; ++k) r.information[k] = k % 7 == 0 ? 1.0 : 0.0;
    if (p->estimate_information) {
        st = reg_information_matrix(w, To, (float)p->information_max_distance, r.information, &r.n_info_pairs);
        if (st != REG_OK) return fail(st);
        r.information_estimated = 1;
    }
    *out = r;
    return REG_OK;
}

reg_status reg_submaps_compute_odometry_constraints(reg_submaps* s, const int32_t* candidates, int32_t n,
                                                    const reg_constraint_params* params, int32_t* n_added) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    if (n_added) *n_added = 0;
    reg_constraint_params def;
    (void)reg_default_odometry_constraint_params(s, 0, &def);
    const reg_constraint_params* p = params ? params : &def;
    if (reg_check_constraint_params(p) != REG_OK || n < 0) {
        h->err = std::string("reg_submaps_compute_odometry_constraints: n < 0, or") + (kSmConstraintMsg + 1);
        return REG_BAD_ARGUMENT;
    }
    std::vector<int32_t> existing, pairs(2 * (s->subs.size() + (size_t)(candidates ? n : 0)) + 2);
    for (const SmConstraint& c : s->odometry) existing.push_back(c.source), existing.push_back(c.target);
    int32_t np = 0;
    if (reg_submaps_odometry_constraint_pairs(s, candidates, candidates ? n : 0, existing.data(), (int32_t)(existing.size() / 2),
                                              pairs.data(), (int32_t)(pairs.size() / 2), &np) != REG_OK) {
        h->err = "reg_submaps_compute_odometry_constraints: an unknown candidate index";
        return REG_BAD_ARGUMENT;
    }
    std::vector<SmConstraint> built((size_t)np);
    for (int32_t k = 0; k < np; ++k) {
        reg_constraint_result r;
        r.struct_size = (int32_t)sizeof(r);
        REGCHK(reg_submaps_build_constraint(s, pairs[2 * k], pairs[2 * k + 1], p, nullptr, &r));
        SmConstraint& c = built[k];
        c.source = r.source;
        c.target = r.target;
        c.flags = (r.information_estimated ? 1 : 0) | 2;   // c.isOdometryConstraint_ = true (constraint_builders.cpp:39)
        std::memcpy(c.T, r.T, sizeof(c.T));
        std::memcpy(c.info, r.information, sizeof(c.info));
    }
    s->odometry.insert(s->odometry.end(), built.begin(), built.end());
    if (n_added) *n_added = np;
    return REG_OK;
}

reg_status reg_submaps_get_odometry_constraints(const reg_submaps* s, int32_t capacity, int32_t* source, int32_t* target, double* T,
                                                double* information, int32_t* flags, int32_t* n_out) {
    if (!s) return REG_BAD_ARGUMENT;
    if (n_out) *n_out = 0;
    const int32_t n = (int32_t)s->odometry.size();
    if ((source || target || T || information || flags) && capacity < n) return REG_BAD_ARGUMENT;
    for (int32_t k = 0; k < n; ++k) {
        const SmConstraint& c = s->odometry[k];
        if (source) source[k] = c.source;
        if (target) target[k] = c.target;
        if (flags) flags[k] = c.flags;
        if (T) std::memcpy(T + 16 * (size_t)k, c.T, sizeof(c.T));
        if (information) std::memcpy(information + 36 * (size_t)k, c.info, sizeof(c.info));
    }
    if (n_out) *n_out = n;
    return REG_OK;
}

reg_status reg_submaps_clear_odometry_constraints(reg_submaps* s) {
    if (!s) return REG_BAD_ARGUMENT;
    s->odometry.clear();
    return REG_OK;
}

reg_status reg_submaps_get_features(reg_submaps* s, int32_t idx, int on_device, double* sparse_xyz64, float* sparse_xyz,
                                    float* sparse_normals, double* fpfh, int64_t capacity_rows, int64_t* n_out) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    if (n_out) *n_out = 0;
    const bool any = sparse_xyz64 || sparse_xyz || sparse_normals || fpfh;
    if (!sm_idx_ok(s, idx) || (any && capacity_rows < s->subs[idx]->n_sparse)) {
        h->err = "reg_submaps_get_features: an unknown submap index, or capacity_rows below the stored rows";
        return REG_BAD_ARGUMENT;
    }
    const SmSubmap& b = *s->subs[idx];
    const int64_t m = b.n_sparse;
    if (n_out) *n_out = m;
    if (!any || m == 0) return REG_OK;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, copy_out(h, sparse_xyz64, b.s_xyz64.p, (size_t)m * 24, on_device));
    HIPCHK(h, copy_out(h, sparse_xyz, b.s_xyz.p, (size_t)m * 12, on_device));
    HIPCHK(h, copy_out(h, sparse_normals, b.s_nrm.p, (size_t)m * 12, on_device));
    HIPCHK(h, copy_out(h, fpfh, b.s_fpfh.p, (size_t)m * 33 * 8, on_device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

reg_status reg_host_registration_consistent(const double T[16], const double bounds[6], int32_t* failed_mask) {
    if (!T || !bounds || !failed_mask) return REG_BAD_ARGUMENT;
    auto R = [&](int r, int c) { return T[4 * c + r]; };
    // Eigen's Quaterniond(Matrix3d)
    double q[4];   // w, x, y, z
    double t = R(0, 0) + R(1, 1) + R(2, 2);
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (R(2, 1) - R(1, 2)) * t;
        q[2] = (R(0, 2) - R(2, 0)) * t;
        q[3] = (R(1, 0) - R(0, 1)) * t;
    } else {
        int i = 0;
        if (R(1, 1) > R(0, 0)) i = 1;
        if (R(2, 2) > R(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R(k, j) - R(j, k)) * t;
        q[1 + j] = (R(j, i) + R(i, j)) * t;
        q[1 + k] = (R(k, i) + R(i, k)) * t;
    }
    const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
    const double v[6] = {std::atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)), std::asin(2.0 * (w * y - x * z)),
                         std::atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z)), T[12], T[13], T[14]};
    int32_t mask = 0;
    for (int k = 0; k < 6; ++k)
        if (std::fabs(v[k]) > bounds[k]) mask |= 1 << k;
    *failed_mask = mask;
    return REG_OK;
}

void reg_loop_closure_struct_sizes(int32_t sizes[2]) {
    if (!sizes) return;
    sizes[0] = (int32_t)sizeof(reg_loop_closure_params);
    sizes[1] = (int32_t)sizeof(reg_loop_closure_verdict);
}

reg_status reg_submaps_build_loop_closure_constraints(reg_submaps* s, int32_t last_finished, int64_t stamp_ns,
                                                      const reg_loop_closure_params* p, reg_loop_closure_verdict* verdicts,
                                                      int32_t capacity, int32_t* n_candidates) {
    if (!s) return REG_BAD_ARGUMENT;
    reg_handle* h = s->h;
    if (n_candidates) *n_candidates = 0;
    if (!p || p->struct_size != (int32_t)sizeof(reg_loop_closure_params) || reg_check_constraint_params(&p->refine) != REG_OK ||
        p->ransac.struct_size != (int32_t)sizeof(reg_ransac_params) || p->ransac.ransac_n < 3 || capacity < 0 ||
        (capacity > 0 && (!verdicts || verdicts[0].struct_size != (int32_t)sizeof(reg_loop_closure_verdict)))) {
        h->err = std::string("reg_submaps_build_loop_closure_constraints: capacity < 0, verdicts missing or of the wrong struct_size, "
                             "ransac of the wrong struct_size or ransac_n < 3, or refine") + kSmConstraintMsg;
        return REG_BAD_ARGUMENT;
    }
    std::vector<int32_t> cand(s->subs.size());
    int32_t nc = 0;
    if (reg_submaps_loop_closure_candidates(s, last_finished, cand.data(), (int32_t)cand.size(), &nc) != REG_OK) {
        h->err = "reg_submaps_build_loop_closure_constraints: an unknown submap index, or one without an entry in the adjacency matrix";
        return REG_BAD_ARGUMENT;
    }
    if (n_candidates) *n_candidates = nc;
    if (nc > capacity) {
        h->err = "reg_submaps_build_loop_closure_constraints: capacity below the number of candidates";
        return REG_BAD_ARGUMENT;
    }
    if (nc == 0) return REG_OK;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    reg_handle* w = nullptr;
    REGCHK(sm_constraint_handle(s, REG_COST_O3D_P2P, &w));
    const SmSubmap& src = *s->subs[last_finished];
    std::vector<reg_loop_closure_verdict> out((size_t)nc);
    for (int32_t c = 0; c < nc; ++c) {
        const SmSubmap& tgt = *s->subs[cand[c]];
        reg_loop_closure_verdict& v = out[c];
        std::memset(&v, 0, sizeof(v));
        v.struct_size = (int32_t)sizeof(v);
        v.source = last_finished;
        v.candidate = cand[c];
        v.stamp_ns = stamp_ns;
        od_identity(v.T_ransac);
        const int64_t na = src.n_sparse, nb = tgt.n_sparse;
        if (na > 0 && nb > 0) {   // RegistrationRANSACBasedOnFeatureMatching (PlaceRecognition.cpp:81-84)
            HIPCHK(h, hipSetDevice(h->prm.device));
            HIPCHK(h, s->lc_ab.reserve((size_t)na * 4));
            HIPCHK(h, s->lc_ba.reserve((size_t)nb * 4));
            HIPCHK(h, s->lc_cor.reserve((size_t)na * 8));
            HIPCHK(h, s->lc_inl.reserve((size_t)na * 8));
            int64_t k = 0;
            reg_status st = reg_match_features(w, src.s_fpfh.as<double>(), na, tgt.s_fpfh.as<double>(), nb, 33, 1,
                                               s->lc_ab.as<int32_t>(), s->lc_ba.as<int32_t>(), s->lc_cor.as<int32_t>(), &k);
            if (st != REG_OK) {
                h->err = std::string("reg_submaps_build_loop_closure_constraints: ") + w->err;
                return st;
            }
            if (k < p->ransac.ransac_n) {   // Open3D's fall-back: every (a, nearest b)
                std::vector<int32_t> ab((size_t)na), pairs(2 * (size_t)na);
                HIPCHK(h, hipMemcpyAsync(ab.data(), s->lc_ab.p, (size_t)na * 4, hipMemcpyDeviceToHost, h->stream));
                HIPCHK(h, hipStreamSynchronize(h->stream));
                for (int64_t a = 0; a < na; ++a) pairs[2 * a] = (int32_t)a, pairs[2 * a + 1] = ab[a];
                HIPCHK(h, hipMemcpyAsync(s->lc_cor.p, pairs.data(), (size_t)na * 8, hipMemcpyHostToDevice, h->stream));
                HIPCHK(h, hipStreamSynchronize(h->stream));
                k = na;
            }
            reg_ransac_result rr;
            std::memset(&rr, 0, sizeof(rr));
            rr.struct_size = (int32_t)sizeof(rr);
            st = reg_ransac_correspondences(w, src.s_xyz64.as<double>(), na, tgt.s_xyz64.as<double>(), nb, s->lc_cor.as<int32_t>(), k,
                                            1, &p->ransac, &rr, s->lc_inl.as<int32_t>(), nullptr);
            if (st != REG_OK) {
                h->err = std::string("reg_submaps_build_loop_closure_constraints: ") + w->err;
                return st;
            }
            std::memcpy(v.T_ransac, rr.T, sizeof(rr.T));
            v.n_correspondences = rr.n_inliers;
            v.ransac_iterations = rr.n_iterations;
            v.ransac_fitness = rr.fitness;
            v.ransac_inlier_rmse = rr.inlier_rmse;
        }
        if (v.n_correspondences < (int64_t)p->ransac_min_correspondence_set_size) {
            v.verdict = REG_LC_RANSAC_SET_TOO_SMALL;
            continue;
        }
        (void)reg_host_registration_consistent(v.T_ransac, p->consistency_bounds, &v.ransac_failed_mask);
        if (v.ransac_failed_mask) {
            v.verdict = REG_LC_RANSAC_INCONSISTENT;
            continue;
        }
        v.constraint.struct_size = (int32_t)sizeof(v.constraint);
        REGCHK(reg_submaps_build_constraint(s, last_finished, cand[c], &p->refine, v.T_ransac, &v.constraint));
        v.refined = 1;
        if (v.constraint.fitness < p->min_refinement_fitness) {
            v.verdict = REG_LC_FITNESS_TOO_LOW;
            continue;
        }
        (void)reg_host_registration_consistent(v.constraint.T, p->consistency_bounds, &v.icp_failed_mask);
        v.verdict = v.icp_failed_mask ? REG_LC_ICP_INCONSISTENT : REG_LC_ACCEPTED;
    }
    std::memcpy(verdicts, out.data(), (size_t)nc * sizeof(reg_loop_closure_verdict));
    return REG_OK;
}

}  // extern "C"
