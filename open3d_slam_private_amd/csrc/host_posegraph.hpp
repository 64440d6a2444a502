// host_posegraph.hpp -- pose-graph optimisation on the device: o3d_slam::OptimizationProblem::solve =
// Open3D's GlobalOptimization (Levenberg-Marquardt with line processes, prune, second pass, reference compensation).  The
// graph lives on the host inside the object; a pass uploads it, runs every kernel of kernels_posegraph.hpp on the handle's
// stream, reads one small record back per LM step and takes the LM decisions on the host, line for line as the contract
// in include/o3dslam_reg.h states them.  A pass that fails leaves the graph as it was.
// Part of the single translation unit reg_core.hip (included there, after host_odometry.hpp; not a standalone header).
#pragma once

struct PgGraph {
    int n = 0;
    std::vector<double> pose, X, info, conf;
    std::vector<int32_t> src, tgt, unc, id;   // id: the edge's index in the list reg_pose_graph_set received
    int edges() const { return (int)src.size(); }
};

struct reg_pose_graph {
    reg_handle* h = nullptr;
    reg_pose_graph_params prm;
    PgGraph g;
    // edges; poses, zeta and e^T L e of the state and of the trial (two sides, swapped on an accepted step); terms, records;
    // the incidence lists; H, the padded factor, b, the working vectors of the substitutions, the step, the pose vector;
    // the step's record and the pivot word
    DevBuf src, tgt, unc, X, info, conf, pose[2], zeta[2], ele[2], term, rec, blk_ptr, blk_item, node_ptr, node_item, H, L, b, w,
        y, delta, x, out, pivot;
    Pinned<double> host_rec;
    int64_t rows_held = 0;
};

static inline int pg_padded(int M) { return (M + kPgTile - 1) / kPgTile * kPgTile; }

// Enqueues the whole solve of (A + lambda I) x = b: A is M x M on the device, L (Mp x Mp), w, y, x (Mp each) its working set
static void pg_solve_enqueue(hipStream_t s, const double* A, int M, int Mp, double lambda, const double* b, double* L, double* w,
                             double* y, double* x, int32_t* pivot) {
    k_pg_load<<<grid_for((int64_t)Mp * Mp), 256, 0, s>>>(A, M, Mp, lambda, b, L, w, pivot);
    const int P = Mp / kPgNB;
    for (int p = 0; p < P; ++p) {
        k_pg_potrf<<<1, 256, 0, s>>>(L, Mp, p, pivot);
        const int start = (p + 1) * kPgNB, below = Mp - start;
        if (below <= 0) continue;
        k_pg_trsm<<<(below + kPgTile - 1) / kPgTile, 256, 0, s>>>(L, Mp, p);
        const int tile0 = start / kPgTile, T = Mp / kPgTile - tile0;
        k_pg_trailing<<<T * (T + 1) / 2, 256, 0, s>>>(L, Mp, p, tile0);
    }
    for (int p = 0; p < P; ++p) {
        const int below = Mp - (p + 1) * kPgNB;
        k_pg_forward<<<std::max(1, (below + 63) / 64), 256, 0, s>>>(L, Mp, p, w, y);
    }
    for (int p = P - 1; p >= 0; --p) k_pg_backward<<<std::max(1, (p * kPgNB + 255) / 256), 256, 0, s>>>(L, Mp, p, y, x);
}

static reg_status pg_pivot_error(reg_handle* h, const char* who, int32_t word) {
    h->err = std::string(who) + ": the pivot of row " + std::to_string(word - 1) + " of the Cholesky factorisation is not positive and finite";
    return REG_BAD_TRANSFORM;
}

static bool pg_params_ok(const reg_pose_graph_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(reg_pose_graph_params)) return false;
    const double v[] = {p->max_correspondence_distance, p->preference_loop_closure, p->edge_prune_threshold,
                        p->min_relative_increment, p->min_relative_residual_increment, p->min_right_term, p->min_residual,
                        p->upper_scale_factor, p->lower_scale_factor};
    for (double x : v)
        if (!std::isfinite(x)) return false;
    return p->max_correspondence_distance >= 0.0 && p->preference_loop_closure >= 0.0 && p->max_iteration >= 0 &&
           p->max_iteration_lm >= 1 && p->lower_scale_factor > 0.0 && p->upper_scale_factor >= p->lower_scale_factor;
}

// Uploads the graph, sizes the working set and builds the incidence lists (once per graph)
static reg_status pg_upload(reg_pose_graph* o, const PgGraph& g) {
    reg_handle* h = o->h;
    const int n = g.n, E = g.edges(), M = 6 * n, Mp = pg_padded(M);
    const size_t e = (size_t)std::max(E, 1);
    HIPCHK(h, o->src.reserve(e * 4));
    HIPCHK(h, o->tgt.reserve(e * 4));
    HIPCHK(h, o->unc.reserve(e * 4));
    HIPCHK(h, o->X.reserve(e * 128));
    HIPCHK(h, o->info.reserve(e * 288));
    HIPCHK(h, o->conf.reserve(e * 8));
    HIPCHK(h, o->term.reserve(e * 8));
    HIPCHK(h, o->rec.reserve(e * kPgRec * 8));
    for (int k = 0; k < 2; ++k) {
        HIPCHK(h, o->pose[k].reserve((size_t)n * 128));
        HIPCHK(h, o->zeta[k].reserve(e * 48));
        HIPCHK(h, o->ele[k].reserve(e * 8));
    }
    HIPCHK(h, o->H.reserve((size_t)M * M * 8));
    HIPCHK(h, o->L.reserve((size_t)Mp * Mp * 8));
    for (DevBuf* v : {&o->b, &o->w, &o->y, &o->delta, &o->x}) HIPCHK(h, v->reserve((size_t)Mp * 8));
    HIPCHK(h, o->out.reserve(kPgRecord * 8));
    HIPCHK(h, o->pivot.reserve(16));
    if (!o->host_rec.p) HIPCHK(h, o->host_rec.alloc(kPgRecord * 8, hipHostMallocDefault));
    o->rows_held = std::max<int64_t>(o->rows_held, Mp);
    // incidence: per block (s, s) (s, t) (t, s) (t, t) of every edge, per node s and t, both in edge order
    std::vector<int32_t> bp((size_t)n * n + 1, 0), np_((size_t)n + 1, 0), bi((size_t)4 * e), ni((size_t)2 * e);
    auto blk = [&](int a, int b) { return (size_t)a * n + b; };
    for (int k = 0; k < E; ++k) {
        const int s = g.src[k], t = g.tgt[k];
        bp[blk(s, s) + 1]++, bp[blk(s, t) + 1]++, bp[blk(t, s) + 1]++, bp[blk(t, t) + 1]++;
        np_[s + 1]++, np_[t + 1]++;
    }
    for (size_t k = 0; k < (size_t)n * n; ++k) bp[k + 1] += bp[k];
    for (int k = 0; k < n; ++k) np_[k + 1] += np_[k];
    {
        std::vector<int32_t> bc(bp.begin(), bp.end() - 1), nc(np_.begin(), np_.end() - 1);
        for (int k = 0; k < E; ++k) {
            const int s = g.src[k], t = g.tgt[k];
            bi[bc[blk(s, s)]++] = 4 * k + 0;
            bi[bc[blk(s, t)]++] = 4 * k + 1;
            bi[bc[blk(t, s)]++] = 4 * k + 2;
            bi[bc[blk(t, t)]++] = 4 * k + 3;
            ni[nc[s]++] = 2 * k + 0;
            ni[nc[t]++] = 2 * k + 1;
        }
    }
    HIPCHK(h, o->blk_ptr.reserve(bp.size() * 4));
    HIPCHK(h, o->blk_item.reserve(bi.size() * 4));
    HIPCHK(h, o->node_ptr.reserve(np_.size() * 4));
    HIPCHK(h, o->node_item.reserve(ni.size() * 4));
    auto up = [&](DevBuf& d, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
    };
    HIPCHK(h, up(o->blk_ptr, bp.data(), bp.size() * 4));
    HIPCHK(h, up(o->blk_item, bi.data(), (size_t)4 * E * 4));
    HIPCHK(h, up(o->node_ptr, np_.data(), np_.size() * 4));
    HIPCHK(h, up(o->node_item, ni.data(), (size_t)2 * E * 4));
    HIPCHK(h, up(o->src, g.src.data(), (size_t)E * 4));
    HIPCHK(h, up(o->tgt, g.tgt.data(), (size_t)E * 4));
    HIPCHK(h, up(o->unc, g.unc.data(), (size_t)E * 4));
    HIPCHK(h, up(o->X, g.X.data(), (size_t)E * 128));
    HIPCHK(h, up(o->info, g.info.data(), (size_t)E * 288));
    HIPCHK(h, up(o->conf, g.conf.data(), (size_t)E * 8));
    HIPCHK(h, up(o->pose[0], g.pose.data(), (size_t)n * 128));
    HIPCHK(h, hipMemsetAsync(o->delta.p, 0, (size_t)Mp * 8, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the host vectors above go out of scope
    return REG_OK;
}

// The launches of a pass, on the object's buffers
struct PgRun {
    reg_pose_graph* o;
    reg_handle* h;
    int n, E, M, Mp;
    double w;
    PgEdges edges() const {
        return PgEdges{o->src.as<int32_t>(), o->tgt.as<int32_t>(), o->unc.as<int32_t>(), o->X.as<double>(), o->info.as<double>()};
    }
    void linearise(int side) const {   // zeta, e^T L e, terms and records at pose[side]
        if (E)
            k_pg_edge<true><<<grid_for(E, 64), 64, 0, h->stream>>>(edges(), E, o->pose[side].as<double>(), o->conf.as<double>(), w,
                                                                 o->zeta[side].as<double>(), o->ele[side].as<double>(),
                                                                 o->term.as<double>(), o->rec.as<double>());
    }
    void trial(int side) const {
        if (E)
            k_pg_edge<false><<<grid_for(E, 64), 64, 0, h->stream>>>(edges(), E, o->pose[side].as<double>(), o->conf.as<double>(), w,
                                                                  o->zeta[side].as<double>(), o->ele[side].as<double>(),
                                                                  o->term.as<double>(), nullptr);
    }
    void confidences(int side) const {
        if (E) k_pg_conf<<<grid_for(E), 256, 0, h->stream>>>(edges(), E, o->ele[side].as<double>(), w, o->conf.as<double>());
    }
    void assemble() const {
        k_pg_assemble<<<grid_for((int64_t)M * M + M), 256, 0, h->stream>>>(n, o->blk_ptr.as<int32_t>(), o->blk_item.as<int32_t>(),
                                                                         o->node_ptr.as<int32_t>(), o->node_item.as<int32_t>(),
                                                                         o->rec.as<double>(), o->conf.as<double>(),
                                                                         o->H.as<double>(), o->b.as<double>());
    }
    void pose_vector(int side) const {
        k_pg_nodes<<<grid_for(n), 256, 0, h->stream>>>(n, o->pose[side].as<double>(), nullptr, nullptr, o->x.as<double>());
    }
    void step(int from, int to) const {
        k_pg_nodes<<<grid_for(n), 256, 0, h->stream>>>(n, o->pose[from].as<double>(), o->delta.as<double>(),
                                                     o->pose[to].as<double>(), nullptr);
    }
    void solve(double lambda) const {
        pg_solve_enqueue(h->stream, o->H.as<double>(), M, Mp, lambda, o->b.as<double>(), o->L.as<double>(), o->w.as<double>(),
                         o->y.as<double>(), o->delta.as<double>(), o->pivot.as<int32_t>());
    }
    reg_status record(double lambda, const double** rec) const {   // the one read-back of a step
        k_pg_scalars<<<1, 256, 0, h->stream>>>(E, M, o->term.as<double>(), o->H.as<double>(), o->b.as<double>(),
                                              o->delta.as<double>(), o->x.as<double>(), lambda, o->pivot.as<int32_t>(),
                                              o->out.as<double>());
        HIPCHK(h, hipMemcpyAsync(o->host_rec.p, o->out.p, kPgRecord * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
        *rec = o->host_rec.p;
        return REG_OK;
    }
};

static reg_status pg_begin(reg_pose_graph* o, const PgGraph& g, PgRun* run) {
    reg_handle* h = o->h;
    if (g.n <= 0) {
        h->err = "pose graph: no graph has been set";
        return REG_NOT_CONFIGURED;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    REGCHK(pg_upload(o, g));
    const int E = g.edges();
    *run = PgRun{o, h, g.n, E, 6 * g.n, pg_padded(6 * g.n),
                 pg_line_process_weight(g.info.data() + 35, E, 36, o->prm.preference_loop_closure,
                                        o->prm.max_correspondence_distance)};
    HIPCHK(h, hipMemsetAsync(o->pivot.p, 0, 16, h->stream));
    return REG_OK;
}

// One LM pass on g; on success g's poses and confidences are the optimised ones
static reg_status pg_pass(reg_pose_graph* o, PgGraph& g, reg_pose_graph_result* res) {
    reg_handle* h = o->h;
    const reg_pose_graph_params& p = o->prm;
    PgRun r;
    REGCHK(pg_begin(o, g, &r));
    const double* rec = nullptr;
    int cur = 0, stop = REG_PG_STOP_NONE, solves = 0, accepted = 0, outer = 0;
    r.linearise(cur);       // zeta and the residual with the confidences of entry
    r.confidences(cur);
    r.assemble();
    r.pose_vector(cur);
    REGCHK(r.record(0.0, &rec));
    double current = rec[0], lambda = 1e-5 * rec[1], nu = 2.0;
    const double first = current;
    if (rec[2] < p.min_right_term) stop = REG_PG_STOP_RIGHT_TERM;
    for (int iter = 0; !stop; ++iter) {
        ++outer;
        int lm_count = 0;
        double rho = 0.0;
        do {
            r.solve(lambda);
            r.step(cur, cur ^ 1);
            r.trial(cur ^ 1);
            REGCHK(r.record(lambda, &rec));
            ++solves;
            if (rec[6] != 0.0) return pg_pivot_error(h, "reg_pose_graph_optimize", (int32_t)rec[6]);
            if (rec[3] < p.min_relative_increment * (rec[4] + p.min_relative_increment)) {
                stop = REG_PG_STOP_INCREMENT;
                break;
            }
            const double fresh = rec[0];
            rho = (current - fresh) / (rec[5] + 1e-3);
            if (rho > 0.0) {
                if (current - fresh < p.min_relative_residual_increment * current) {
                    stop = REG_PG_STOP_RESIDUAL_INCREMENT;
                    break;
                }
                const double c = 2.0 * rho - 1.0;
                lambda *= std::max(p.lower_scale_factor, std::min(p.upper_scale_factor, 1.0 - c * c * c));
                nu = 2.0;
                cur ^= 1;
                current = fresh;
                ++accepted;
                r.pose_vector(cur);
                r.confidences(cur);
                r.linearise(cur);
                r.assemble();
                REGCHK(r.record(lambda, &rec));
                if (rec[2] < p.min_right_term) {
                    stop = REG_PG_STOP_RIGHT_TERM;
                    break;
                }
            } else {
                lambda *= nu;
                nu *= 2.0;
            }
            if (++lm_count >= p.max_iteration_lm) stop = REG_PG_STOP_MAX_ITERATION_LM;
        } while (!(rho > 0.0) && !stop);
        if (stop) break;
        if (current < p.min_residual)
            stop = REG_PG_STOP_MIN_RESIDUAL;
        else if (iter >= p.max_iteration)
            stop = REG_PG_STOP_MAX_ITERATION;
    }
    const int E = g.edges();
    std::vector<double> pose((size_t)g.n * 16), conf((size_t)E);
    HIPCHK(h, hipMemcpyAsync(pose.data(), o->pose[cur].p, pose.size() * 8, hipMemcpyDeviceToHost, h->stream));
    if (E) HIPCHK(h, hipMemcpyAsync(conf.data(), o->conf.p, conf.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    g.pose.swap(pose);
    g.conf.swap(conf);
    res->outer_iterations = outer;
    res->lm_solves = solves;
    res->accepted_steps = accepted;
    res->stop_reason = stop;
    res->valid_edges = 0;
    for (int k = 0; k < E; ++k) res->valid_edges += g.conf[k] > p.edge_prune_threshold;
    res->first_residual = first;
    res->last_residual = current;
    res->last_lambda = lambda;
    res->weight = r.w;
    return REG_OK;
}

// CreatePrunedPoseGraph: every certain edge, and the uncertain ones whose confidence is above the threshold
static void pg_prune(PgGraph& g, double threshold) {
    PgGraph k;
    k.n = g.n;
    k.pose = g.pose;
    for (int e = 0; e < g.edges(); ++e) {
        if (g.unc[e] && !(g.conf[e] > threshold)) continue;
        k.src.push_back(g.src[e]);
        k.tgt.push_back(g.tgt[e]);
        k.unc.push_back(g.unc[e]);
        k.id.push_back(g.id[e]);
        k.conf.push_back(g.conf[e]);
        k.X.insert(k.X.end(), g.X.begin() + 16 * (size_t)e, g.X.begin() + 16 * (size_t)(e + 1));
        k.info.insert(k.info.end(), g.info.begin() + 36 * (size_t)e, g.info.begin() + 36 * (size_t)(e + 1));
    }
    g = std::move(k);
}

static bool pg_result_ok(const reg_pose_graph_result* r) { return r && r->struct_size == (int32_t)sizeof(reg_pose_graph_result); }
static void pg_result_reset(reg_pose_graph_result* r) {
    std::memset(r, 0, sizeof(*r));
    r->struct_size = (int32_t)sizeof(reg_pose_graph_result);
}

extern "C" {

void reg_default_pose_graph_params(reg_pose_graph_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_pose_graph_params);
    p->reference_node = 0;                     // Parameters.hpp:142-147
    p->max_correspondence_distance = 10.0;
    p->preference_loop_closure = 2.0;
    p->edge_prune_threshold = 0.2;
    p->max_iteration = 100;                    // GlobalOptimizationConvergenceCriteria's defaults
    p->max_iteration_lm = 20;
    p->min_relative_increment = 1e-6;
    p->min_relative_residual_increment = 1e-6;
    p->min_right_term = 1e-6;
    p->min_residual = 1e-6;
    p->upper_scale_factor = 2.0 / 3.0;
    p->lower_scale_factor = 1.0 / 3.0;
}

reg_status reg_check_pose_graph_params(const reg_pose_graph_params* p) { return pg_params_ok(p) ? REG_OK : REG_BAD_ARGUMENT; }

void reg_pose_graph_struct_sizes(int32_t sizes[3]) {
    if (!sizes) return;
    sizes[0] = (int32_t)sizeof(reg_pose_graph_params);
    sizes[1] = (int32_t)sizeof(reg_pose_graph_result);
    sizes[2] = (int32_t)sizeof(reg_pose_graph_info);
}

reg_status reg_pose_graph_create(reg_handle* h, const reg_pose_graph_params* p, reg_pose_graph** out) {
    if (!h || !out) return REG_BAD_ARGUMENT;
    *out = nullptr;
    if (!pg_params_ok(p)) {
        h->err = "reg_pose_graph_create: params missing or of the wrong struct_size, a non-finite value, a negative distance, "
                 "preference or max_iteration, max_iteration_lm < 1, or scale factors not 0 < lower <= upper";
        return REG_BAD_ARGUMENT;
    }
    reg_pose_graph* g = new reg_pose_graph();   // holds no device memory until the first pass
    g->h = h;
    g->prm = *p;
    *out = g;
    return REG_OK;
}

void reg_pose_graph_destroy(reg_pose_graph* g) {
    if (!g) return;
    if (g->h->device_ok && hipSetDevice(g->h->prm.device) == hipSuccess) (void)hipStreamSynchronize(g->h->stream);
    delete g;
}

reg_status reg_pose_graph_clear(reg_pose_graph* g) {
    if (!g) return REG_BAD_ARGUMENT;
    g->g = PgGraph();
    return REG_OK;
}

reg_status reg_pose_graph_set(reg_pose_graph* o, const double* poses, int64_t n_nodes, const int32_t* src, const int32_t* tgt,
                              const double* X, const double* info, const int32_t* uncertain, const double* confidence,
                              int64_t n_edges) {
    if (!o) return REG_BAD_ARGUMENT;
    reg_handle* h = o->h;
    auto bad = [&](const char* what) {
        h->err = std::string("reg_pose_graph_set: ") + what;
        return REG_BAD_ARGUMENT;
    };
    if (n_nodes < 1 || n_nodes > REG_POSE_GRAPH_MAX_NODES || !poses) return bad("1 <= n_nodes <= REG_POSE_GRAPH_MAX_NODES with poses");
    if (n_edges < 0 || n_edges > (int64_t)1 << 24 || (n_edges > 0 && (!src || !tgt || !X || !info || !uncertain)))
        return bad("0 <= n_edges <= 2^24 with every edge array for n_edges > 0");
    for (int64_t k = 0; k < n_nodes * 16; ++k)
        if (!std::isfinite(poses[k])) return bad("a pose entry is not finite");
    for (int64_t e = 0; e < n_edges; ++e) {
        if (src[e] < 0 || src[e] >= n_nodes || tgt[e] < 0 || tgt[e] >= n_nodes) return bad("a node id is out of range");
        if (src[e] == tgt[e]) return bad("an edge has source == target");
        if (confidence && !(confidence[e] >= 0.0 && confidence[e] <= 1.0)) return bad("a confidence lies outside [0, 1]");
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(X[16 * e + k])) return bad("an edge transformation is not finite");
        for (int k = 0; k < 36; ++k)
            if (!std::isfinite(info[36 * e + k])) return bad("an information matrix is not finite");
    }
    PgGraph g;
    g.n = (int)n_nodes;
    g.pose.assign(poses, poses + n_nodes * 16);
    g.src.assign(src, src + n_edges);
    g.tgt.assign(tgt, tgt + n_edges);
    g.unc.resize((size_t)n_edges);
    g.id.resize((size_t)n_edges);
    for (int64_t e = 0; e < n_edges; ++e) g.unc[e] = uncertain[e] != 0, g.id[e] = (int32_t)e;
    g.X.assign(X, X + n_edges * 16);
    g.info.assign(info, info + n_edges * 36);
    if (confidence)
        g.conf.assign(confidence, confidence + n_edges);
    else
        g.conf.assign((size_t)n_edges, 1.0);
    o->g = std::move(g);
    return REG_OK;
}

reg_status reg_pose_graph_linearize(reg_pose_graph* o, double* H, double* b, double* zeta, double* residual, double* weight) {
    if (!o) return REG_BAD_ARGUMENT;
    reg_handle* h = o->h;
    PgRun r;
    REGCHK(pg_begin(o, o->g, &r));
    const double* rec = nullptr;
    r.linearise(0);
    r.assemble();
    r.pose_vector(0);
    HIPCHK(h, copy_out(h, H, o->H.p, (size_t)r.M * r.M * 8, 0));
    HIPCHK(h, copy_out(h, b, o->b.p, (size_t)r.M * 8, 0));
    HIPCHK(h, copy_out(h, zeta, o->zeta[0].p, (size_t)r.E * 48, 0));
    REGCHK(r.record(0.0, &rec));
    if (residual) *residual = rec[0];
    if (weight) *weight = r.w;
    return REG_OK;
}

reg_status reg_pose_graph_optimize(reg_pose_graph* o, reg_pose_graph_result* res) {
    if (!o) return REG_BAD_ARGUMENT;
    if (!pg_result_ok(res)) {
        o->h->err = "reg_pose_graph_optimize: result missing or of the wrong struct_size";
        return REG_BAD_ARGUMENT;
    }
    pg_result_reset(res);
    PgGraph work = o->g;
    REGCHK(pg_pass(o, work, res));
    o->g = std::move(work);
    return REG_OK;
}

reg_status reg_pose_graph_global_optimize(reg_pose_graph* o, reg_pose_graph_result res[2]) {
    if (!o) return REG_BAD_ARGUMENT;
    if (!res || !pg_result_ok(&res[0]) || !pg_result_ok(&res[1])) {
        o->h->err = "reg_pose_graph_global_optimize: results missing or of the wrong struct_size";
        return REG_BAD_ARGUMENT;
    }
    pg_result_reset(&res[0]);
    pg_result_reset(&res[1]);
    PgGraph work = o->g;
    REGCHK(pg_pass(o, work, &res[0]));
    pg_prune(work, o->prm.edge_prune_threshold);
    REGCHK(pg_pass(o, work, &res[1]));
    pg_prune(work, o->prm.edge_prune_threshold);
    const int ref = o->prm.reference_node;
    if (ref >= 0 && ref < work.n) {   // CompensateReferencePoseGraphNode
        double inv[16], C[16], P[16];
        pg_rigid_inverse(&work.pose[16 * (size_t)ref], inv);
        pg_mul(&o->g.pose[16 * (size_t)ref], inv, C);
        for (int i = 0; i < work.n; ++i) {
            pg_mul(C, &work.pose[16 * (size_t)i], P);
            std::memcpy(&work.pose[16 * (size_t)i], P, sizeof(P));
        }
    }
    o->g = std::move(work);
    return REG_OK;
}

reg_status reg_pose_graph_get(reg_pose_graph* o, int64_t capacity_nodes, double* poses, int64_t capacity_edges, int32_t* src,
                              int32_t* tgt, double* confidence, int64_t* n_edges) {
    if (!o) return REG_BAD_ARGUMENT;
    const PgGraph& g = o->g;
    if (n_edges) *n_edges = 0;
    if ((poses && capacity_nodes < g.n) || ((src || tgt || confidence) && capacity_edges < g.edges())) {
        o->h->err = "reg_pose_graph_get: a capacity is below the rows of the graph";
        return REG_BAD_ARGUMENT;
    }
    if (poses) std::memcpy(poses, g.pose.data(), g.pose.size() * 8);
    if (src) std::memcpy(src, g.src.data(), g.src.size() * 4);
    if (tgt) std::memcpy(tgt, g.tgt.data(), g.tgt.size() * 4);
    if (confidence) std::memcpy(confidence, g.conf.data(), g.conf.size() * 8);
    if (n_edges) *n_edges = g.edges();
    return REG_OK;
}

reg_status reg_pose_graph_get_edge_ids(reg_pose_graph* o, int64_t capacity_edges, int32_t* ids) {
    if (!o || !ids) return REG_BAD_ARGUMENT;
    if (capacity_edges < o->g.edges()) {
        o->h->err = "reg_pose_graph_get_edge_ids: capacity_edges is below the edges of the graph";
        return REG_BAD_ARGUMENT;
    }
    std::memcpy(ids, o->g.id.data(), o->g.id.size() * 4);
    return REG_OK;
}

reg_status reg_pose_graph_get_info(const reg_pose_graph* o, reg_pose_graph_info* info) {
    if (!o || !info || info->struct_size != (int32_t)sizeof(reg_pose_graph_info)) return REG_BAD_ARGUMENT;
    info->n_nodes = o->g.n;
    info->n_edges = o->g.edges();
    info->n_uncertain = 0;
    for (int32_t u : o->g.unc) info->n_uncertain += u != 0;
    info->solver_rows = o->rows_held;
    info->device_bytes = 0;
    for (const DevBuf* d : {&o->src, &o->tgt, &o->unc, &o->X, &o->info, &o->conf, &o->pose[0], &o->pose[1], &o->zeta[0], &o->zeta[1],
                            &o->ele[0], &o->ele[1], &o->term, &o->rec, &o->blk_ptr, &o->blk_item, &o->node_ptr, &o->node_item, &o->H,
                            &o->L, &o->b, &o->w, &o->y, &o->delta, &o->x, &o->out, &o->pivot})
        info->device_bytes += (int64_t)d->cap;
    return REG_OK;
}

reg_status reg_host_pose_graph_edge(const double Ts[16], const double Tt[16], const double X[16], double zeta[6], double Js[36],
                                    double Jt[36]) {
    if (!Ts || !Tt || !X || !zeta) return REG_BAD_ARGUMENT;
    pg_edge(Ts, Tt, X, zeta, Js, Jt);
    return REG_OK;
}

reg_status reg_host_pose_vector(const double T[16], double x[6]) {
    if (!T || !x) return REG_BAD_ARGUMENT;
    pg_pose_vector(T, x);
    return REG_OK;
}

reg_status reg_host_pose_step(const double delta[6], const double pose[16], double out[16]) {
    if (!delta || !pose || !out || out == pose) return REG_BAD_ARGUMENT;
    pg_pose_step(delta, pose, out);
    return REG_OK;
}

reg_status reg_host_line_process_weight(const double* info, int64_t n_edges, double preference, double max_correspondence_distance,
                                        double* weight) {
    if (!weight || n_edges < 0 || (n_edges > 0 && !info)) return REG_BAD_ARGUMENT;
    *weight = pg_line_process_weight(info ? info + 35 : nullptr, n_edges, 36, preference, max_correspondence_distance);
    return REG_OK;
}

reg_status reg_debug_spd_solve_f64(reg_handle* h, int64_t n, const double* A, const double* b, double* x, int32_t* status) {
    if (!h) return REG_BAD_ARGUMENT;
    if (status) *status = 0;
    if (n < 1 || n > 6 * REG_POSE_GRAPH_MAX_NODES || !A || !b || !x) {
        h->err = "reg_debug_spd_solve_f64: 1 <= n <= 6 * REG_POSE_GRAPH_MAX_NODES with A, b and x";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const int M = (int)n, Mp = pg_padded(M);
    DevBuf dA, db, dL, dw, dy, dx, dp;
    HIPCHK(h, dA.reserve((size_t)M * M * 8));
    HIPCHK(h, dL.reserve((size_t)Mp * Mp * 8));
    for (DevBuf* v : {&db, &dw, &dy, &dx}) HIPCHK(h, v->reserve((size_t)Mp * 8));
    HIPCHK(h, dp.reserve(16));
    HIPCHK(h, hipMemcpyAsync(dA.p, A, (size_t)M * M * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(db.p, b, (size_t)M * 8, hipMemcpyHostToDevice, h->stream));
    pg_solve_enqueue(h->stream, dA.as<double>(), M, Mp, 0.0, db.as<double>(), dL.as<double>(), dw.as<double>(), dy.as<double>(),
                     dx.as<double>(), dp.as<int32_t>());
    int32_t word = 0;
    std::vector<double> sol((size_t)M);
    HIPCHK(h, hipMemcpyAsync(&word, dp.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(sol.data(), dx.p, (size_t)M * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (status) *status = word;
    if (word != 0) return pg_pivot_error(h, "reg_debug_spd_solve_f64", word);
    std::memcpy(x, sol.data(), (size_t)M * 8);
    return REG_OK;
}

}  // extern "C"
