// pose_graph_host_check.cpp -- stand-alone check of the host-only pose-graph exports (no device needed): reads case (c) of
// the pose-graph tests (tests/golden/pose_graph_case_c.txt, written by tests/golden/make_pose_graph_fixture.py) and compares
// reg_host_pose_graph_edge and reg_host_line_process_weight with the recorded values bit for bit, then walks
// reg_host_pose_step and reg_host_pose_vector over every node.  Meant to be built together with the library's translation
// unit under the host sanitizers (`make pose_graph_host_check` here) and run on any machine.
#include "../include/o3dslam_reg.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static bool read_doubles(FILE* f, double* out, int n) {
    for (int k = 0; k < n; ++k)
        if (std::fscanf(f, "%la", &out[k]) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    const char* path = argc > 1 ? argv[1] : "../tests/golden/pose_graph_case_c.txt";
    FILE* f = std::fopen(path, "r");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    int n = 0, E = 0;
    double head[3];
    if (std::fscanf(f, "%d %d", &n, &E) != 2 || n < 1 || E < 0 || !read_doubles(f, head, 3)) return 2;
    std::vector<double> poses((size_t)n * 16), info((size_t)E * 36);
    if (!read_doubles(f, poses.data(), n * 16)) return 2;
    int mismatches = 0;
    for (int e = 0; e < E; ++e) {
        int s = 0, t = 0, u = 0;
        double X[16], want[6 + 72], zeta[6], Js[36], Jt[36];
        if (std::fscanf(f, "%d %d %d", &s, &t, &u) != 3 || s < 0 || s >= n || t < 0 || t >= n) return 2;
        if (!read_doubles(f, X, 16) || !read_doubles(f, &info[(size_t)e * 36], 36) || !read_doubles(f, want, 78)) return 2;
        if (reg_host_pose_graph_edge(&poses[(size_t)s * 16], &poses[(size_t)t * 16], X, zeta, Js, Jt) != REG_OK) return 3;
        for (int k = 0; k < 6; ++k) mismatches += !(zeta[k] == want[k]);
        for (int k = 0; k < 36; ++k) mismatches += !(Js[k] == want[6 + k]) + !(Jt[k] == want[42 + k]);
        if (reg_host_pose_graph_edge(&poses[(size_t)s * 16], &poses[(size_t)t * 16], X, zeta, nullptr, nullptr) != REG_OK) return 3;
    }
    std::fclose(f);
    double w = -1.0;
    if (reg_host_line_process_weight(info.data(), E, head[0], head[1], &w) != REG_OK) return 3;
    mismatches += !(w == head[2]);
    double worst = 0.0;
    for (int i = 0; i < n; ++i) {   // V(x(T)) I = T up to rounding: the pose vector is the inverse map of the pose step
        double x[6], back[16];
        const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (reg_host_pose_vector(&poses[(size_t)i * 16], x) != REG_OK || reg_host_pose_step(x, eye, back) != REG_OK) return 3;
        for (int k = 0; k < 16; ++k) worst = std::fmax(worst, std::fabs(back[k] - poses[(size_t)i * 16 + k]));
    }
    std::printf("%d nodes, %d edges: %d mismatches, weight %.17g, |V(x(T)) - T| <= %.3g\n", n, E, mismatches, w, worst);
    return mismatches == 0 && worst <= 1e-12 ? 0 : 1;
}
