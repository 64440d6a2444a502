"""A literal Python restatement of the reference code behind reg_submaps (include/o3dslam_reg.h), with sets and
dicts: VoxelMap's occupancy set and SubmapCollection::isSwitchingSubmapsConsistant, AdjacencyMatrix, SubmapCollection
(insertScan, updateActiveSubmap, createNewSubmap, findClosestSubmap, forceNewSubmapCreation, transform),
PlaceRecognition::getLoopClosureCandidatesIdxs and the pair selection of computeOdometryConstraints.  float64 scalars and
numpy's elementwise operators: one rounding per operation, no contraction.

The map of a submap is an object supplied by the caller (`new_map()`), with insert_scan(raw, xyz, T, nrm, cov, perform_carving),
set(xyz, nrm, cov, voxel), transform(T), get_center(), n_rows() and points(): tests/map_cloud_restatement.MapCloud on the
CPU, capi.MapCloud on the device (tests/submaps_cases.py wraps both)."""
import math
from collections import deque

import numpy as np

LIMIT = 1 << 20
INT_MAX = 2 ** 31 - 1
KEEP, SWITCH, CREATE, NEED_FITNESS, SET_FORCE_FLAG, FORCED = 0, 1, 2, 3, 4, 8


# ---- VoxelMap: the occupancy set (VoxelHashMap.hpp:43-51,115-119; Voxel.cpp:123-134) ---------------------------------------
def voxel_indices(xyz, voxel):
    """floor(p * (1 / voxel)) per axis as float64, and the rows that get a key: finite and within +-(2^20 - 1) (the
    departure: a row beyond that gets no key)."""
    inv = np.float64(1.0) / np.float64(voxel)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(xyz, np.float64).reshape(-1, 3) * inv)
        ok = np.all(np.abs(f) < LIMIT, axis=1)          # false for NaN
    return f, ok


def pack(f):
    """The 64-bit key of integer indices (n x 3): offset binary, z most significant."""
    i = f.astype(np.int64) + LIMIT
    return (i[:, 2].astype(np.uint64) << np.uint64(42)) | (i[:, 1].astype(np.uint64) << np.uint64(21)) | i[:, 0].astype(np.uint64)


def occupancy_set(xyz, voxel):
    """voxelMap_.insertCloud: the set of keys of the rows."""
    f, ok = voxel_indices(xyz, voxel)
    return set(int(k) for k in pack(f[ok]))


def transform_rigid(T, xyz):
    """mapToRangeSensor * p: each row ((R0 x + R1 y) + R2 z) + t, no division."""
    T = np.asarray(T, np.float64)
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def switch_fitness(keys, scan_xyz, T, voxel):
    """isSwitchingSubmapsConsistant (SubmapCollection.cpp:390-402): (count, fitness); 0 / 0 is NaN."""
    n = len(scan_xyz)
    count = 0
    if n:
        f, ok = voxel_indices(transform_rigid(T, scan_xyz), voxel)
        count = sum(1 for k in pack(f[ok]) if int(k) in keys)
    return count, (np.float64(count) / np.float64(n) if n else float("nan"))


# ---- AdjacencyMatrix.cpp ---------------------------------------------------------------------------------------------------
class AdjacencyMatrix:
    def __init__(self):
        self.adjacency_ = {}
        self.isLoopClosureSubmap_ = {}

    def addEdge(self, id1, id2):
        self.adjacency_.setdefault(id1, set()).add(id2)
        self.adjacency_.setdefault(id2, set()).add(id1)
        self.isLoopClosureSubmap_[id1] = False
        self.isLoopClosureSubmap_[id2] = False

    def markAsLoopClosureSubmap(self, id):
        if id not in self.isLoopClosureSubmap_:
            raise KeyError(id)
        self.isLoopClosureSubmap_[id] = True

    def isAdjacent(self, id1, id2):
        if id1 == id2:
            return True
        return id2 in self.adjacency_.get(id1, ())

    def getDistanceToNearestLoopClosureSubmap(self, id):
        if not self.isLoopClosureSubmap_:
            return INT_MAX
        toProcess, visited, parents = deque([id]), {id}, {}
        v = id
        while toProcess:
            v = toProcess.popleft()
            if self.isLoopClosureSubmap_[v]:          # .at(v): KeyError as the reference throws
                break
            for adj in sorted(self.adjacency_[v]):    # std::set: ascending
                if adj not in visited:
                    visited.add(adj)
                    toProcess.append(adj)
                    parents[adj] = v
        distance = 0
        while v != id:
            v = parents[v]
            distance += 1
        return max(0, distance - 1)

    def matrix(self, n):
        adj, marks = np.zeros((n, n), np.uint8), np.full(n, -1, np.int32)
        for a, s in self.adjacency_.items():
            for b in s:
                adj[a, b] = 1
        for a, m in self.isLoopClosureSubmap_.items():
            marks[a] = int(m)
        return adj, marks


# ---- updateActiveSubmap's branch table (SubmapCollection.cpp:94-148) ---------------------------------------------------------
def decide_path(force_flag, scans_in_active, min_num_range_data, is_use_initial_map, active_points, max_num_points,
                closest_is_active, distance_to_closest, distance_to_active, radius, adjacent, fitness_ok):
    """(the bits reg_host_submaps_decide returns, the name of the branch taken); fitness_ok: True / False, or None where it is
    not known yet."""
    if force_flag:
        return CREATE | FORCED, "forced"
    if scans_in_active < min_num_range_data:
        return KEEP, "few_scans"
    if is_use_initial_map:
        return KEEP, "initial_map"
    flag = SET_FORCE_FLAG if active_points > max_num_points else 0
    isAnotherSubmapWithinRange = distance_to_closest < radius
    if isAnotherSubmapWithinRange:
        if closest_is_active:
            return KEEP | flag, "closest_is_active"
        name = "not_adjacent"
        if adjacent:
            if fitness_ok is None:
                return NEED_FITNESS | flag, "need_fitness"
            if fitness_ok:
                return SWITCH | flag, "revisit_switch"
            name = "revisit_failed"
        isTraveledSufficientDistance = distance_to_active > radius
        return (CREATE if isTraveledSufficientDistance else KEEP) | flag, name + ("_create" if isTraveledSufficientDistance else "_keep")
    return CREATE | flag, "out_of_range_create"


BRANCHES = ("forced", "few_scans", "initial_map", "closest_is_active", "revisit_switch", "revisit_failed_create",
            "revisit_failed_keep", "not_adjacent_create", "not_adjacent_keep", "out_of_range_create")


def decide(*args):
    return decide_path(*args)[0]


def norm3(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


# ---- Submap / SubmapCollection ------------------------------------------------------------------------------------------------
class Submap:
    def __init__(self, id, parentId, mapToSubmap, map_object):
        self.id_, self.parentId_ = id, parentId
        self.mapToSubmap_ = np.array(mapToSubmap, np.float64)
        self.mapToRangeSensor_ = np.eye(4)
        self.submapCenter_ = np.zeros(3)
        self.isCenterComputed_ = False
        self.voxelMap_ = set()
        self.feature_ = False
        self.featureClock_ = 0.0
        self.map = map_object

    def getMapToSubmapCenter(self):
        return self.submapCenter_ if self.isCenterComputed_ else self.mapToSubmap_[:3, 3]


class SubmapCollection:
    """p: dict(radius, min_num_range_data, max_num_points, num_scans_overlap, revisit_min_fitness, is_use_initial_map,
    is_carving_enabled, map_voxel, factor, min_seconds_between_features, loop_closure_search_radius,
    min_submaps_between_loop_closures)."""

    def __init__(self, p, new_map):
        assert p["num_scans_overlap"] > 0, "Num scan overlap has to be > 0"
        self.p, self.new_map = p, new_map
        self.submaps_, self.adjacencyMatrix_ = [], AdjacencyMatrix()
        self.activeSubmapIdx_, self.submapId_, self.numScansMergedInActiveSubmap_ = 0, 0, 0
        self.lastFinishedSubmapIdx_ = 0
        self.isForceNewSubmapCreation_ = False
        self.mapToRangeSensor_, self.timestamp_ = np.eye(4), 0
        self.overlapScansBuffer_ = deque()
        self.finishedSubmapsIdxs_, self.loopClosureCandidatesIdxs_ = [], []
        self.log = []                                   # (decision bits, fitness or None) per updateActiveSubmap
        self.branches = []                              # and the name of its branch
        self.createNewSubmap(self.mapToRangeSensor_)

    @property
    def occupancy_voxel(self):
        return np.float64(self.p["factor"]) * np.float64(self.p["map_voxel"])

    def createNewSubmap(self, mapToSubmap):
        submapId = self.submapId_
        self.submapId_ += 1
        self.submaps_.append(Submap(submapId, self.activeSubmapIdx_, mapToSubmap, self.new_map()))
        self.activeSubmapIdx_ = len(self.submaps_) - 1
        self.numScansMergedInActiveSubmap_ = 0

    def findClosestSubmap(self, T):
        p0 = T[:3, 3]
        best = 0
        for i in range(1, len(self.submaps_)):          # std::min_element: the first minimum
            if norm3(p0, self.submaps_[i].getMapToSubmapCenter()) < norm3(p0, self.submaps_[best].getMapToSubmapCenter()):
                best = i
        return best

    def isSwitchingSubmapsConsistant(self, scan, candidate, T):
        count, fitness = switch_fitness(self.submaps_[candidate].voxelMap_, scan[0], T, self.occupancy_voxel)
        self.last_fitness = (count, fitness)
        return bool(fitness > self.p["revisit_min_fitness"])

    def updateActiveSubmap(self, T, scan):
        p = self.p
        closest = self.findClosestSubmap(self.mapToRangeSensor_)
        active = self.submaps_[self.activeSubmapIdx_]
        pos = self.mapToRangeSensor_[:3, 3]
        args = (self.isForceNewSubmapCreation_, self.numScansMergedInActiveSubmap_, p["min_num_range_data"],
                p["is_use_initial_map"], active.map.n_rows(), p["max_num_points"], closest == self.activeSubmapIdx_,
                norm3(pos, self.submaps_[closest].getMapToSubmapCenter()), norm3(pos, active.getMapToSubmapCenter()), p["radius"],
                self.adjacencyMatrix_.isAdjacent(self.submaps_[closest].id_, active.id_))
        self.last_fitness = None
        d, name = decide_path(*args, None)
        if d & 3 == NEED_FITNESS:
            d, name = decide_path(*args, self.isSwitchingSubmapsConsistant(scan, closest, T))
        self.log.append((d, self.last_fitness))
        self.branches.append(name)
        if d & FORCED:
            self.isForceNewSubmapCreation_ = False
        if d & SET_FORCE_FLAG:
            self.isForceNewSubmapCreation_ = True
        if d & 3 == SWITCH:
            self.activeSubmapIdx_ = closest
        elif d & 3 == CREATE:
            self.createNewSubmap(self.mapToRangeSensor_)
        return d

    def _submap_insert(self, submap, raw, scan, T, carve):
        """Submap::insertScan (Submap.cpp:39-96)."""
        xyz, nrm, cov = scan
        if len(xyz) == 0:
            return None
        submap.mapToRangeSensor_ = np.array(T, np.float64)
        if self.p["is_use_initial_map"] and submap.map.n_rows() == 0:
            submap.map.set(xyz, nrm, cov, self.p["map_voxel"])
            return None
        return submap.map.insert_scan(raw, xyz, T, nrm, cov, bool(carve and self.p["is_carving_enabled"]))

    def insertScan(self, raw, scan, T, timestamp):
        """scan = (xyz, normals or None, covs or None) in the sensor frame."""
        T = np.array(T, np.float64)
        self.mapToRangeSensor_, self.timestamp_ = T, timestamp
        prev = self.activeSubmapIdx_
        self.overlapScansBuffer_.append((scan, timestamp, T))
        while len(self.overlapScansBuffer_) > self.p["num_scans_overlap"]:
            self.overlapScansBuffer_.popleft()
        self.updateActiveSubmap(T, scan)
        result = None
        if prev != self.activeSubmapIdx_:
            result = self._submap_insert(self.submaps_[prev], raw, scan, T, True)
            self.submaps_[prev].submapCenter_ = self.submaps_[prev].map.get_center()
            self.submaps_[prev].isCenterComputed_ = True
            self.lastFinishedSubmapIdx_ = prev
            self.finishedSubmapsIdxs_.append((prev, timestamp))
            self.numScansMergedInActiveSubmap_ = 0
            self.adjacencyMatrix_.addEdge(self.submaps_[prev].id_, self.submaps_[self.activeSubmapIdx_].id_)
            while self.overlapScansBuffer_:
                s, _, Ts = self.overlapScansBuffer_.popleft()
                self._submap_insert(self.submaps_[self.activeSubmapIdx_], s[0], s, Ts, False)
        else:
            result = self._submap_insert(self.submaps_[self.activeSubmapIdx_], raw, scan, T, True)
        self.numScansMergedInActiveSubmap_ += 1
        return result

    def forceNewSubmapCreation(self):
        self.isForceNewSubmapCreation_ = True
        empty = (np.zeros((0, 3)), None, None)
        self.insertScan(np.zeros((0, 3)), empty, self.mapToRangeSensor_, self.timestamp_)
        self.isForceNewSubmapCreation_ = False

    def computeFeatures(self, idx, now):
        """The gate and the voxel map of Submap::computeFeatures (Submap.cpp:255-275)."""
        s = self.submaps_[idx]
        if s.feature_ and now - s.featureClock_ < self.p["min_seconds_between_features"]:
            return False
        s.voxelMap_ = occupancy_set(s.map.points(), self.occupancy_voxel)
        s.feature_, s.featureClock_ = True, now
        return True

    def updateAdjacencyMatrix(self, pairs):
        for a, b in pairs:
            self.adjacencyMatrix_.addEdge(a, b)
            self.adjacencyMatrix_.markAsLoopClosureSubmap(a)
            self.adjacencyMatrix_.markAsLoopClosureSubmap(b)

    def transform(self, increments):
        """increments: [(submapId, dT)] (SubmapCollection.cpp:322-373).  Returns {submap index: [positions applied]}."""
        applied = {}
        optimizedIdxs = []
        for i, (sid, dT) in enumerate(increments):
            if sid < len(self.submaps_):
                self._submap_transform(self.submaps_[sid], dT)
                applied.setdefault(sid, []).append(i)
                optimizedIdxs.append(sid)
        toUpdate = [i for i in range(len(self.submaps_)) if i not in set(optimizedIdxs)]
        for idx in toUpdate:
            cur = idx
            while increments:
                cur = self.submaps_[cur].parentId_
                if cur not in toUpdate:
                    if cur >= len(increments):
                        raise IndexError("transformIncrements.at")
                    self._submap_transform(self.submaps_[idx], increments[cur][1])
                    applied.setdefault(idx, []).append(cur)
                    break
                if cur == self.submaps_[cur].parentId_:
                    raise RuntimeError("Stuck in a loop, this should not happen")
        self.overlapScansBuffer_.clear()
        return applied

    @staticmethod
    def _submap_transform(s, T):
        T = np.asarray(T, np.float64)
        s.map.transform(T)
        s.mapToRangeSensor_ = mul44(s.mapToRangeSensor_, T)
        c = s.submapCenter_
        s.submapCenter_ = np.array([((T[r, 0] * c[0] + T[r, 1] * c[1]) + T[r, 2] * c[2]) + T[r, 3] for r in range(3)])


def transform_plan(parents, ids):
    """Which position of the list each submap receives (the last one for a listed id), -1 for none; raises as the reference."""
    n = len(parents)
    plan = [-1] * n
    listed = set()
    for k, sid in enumerate(ids):
        if 0 <= sid < n:
            plan[sid] = k
            listed.add(sid)
    if not len(ids):
        return plan
    for idx in range(n):
        if idx in listed:
            continue
        cur = idx
        while True:
            cur = parents[cur]
            if cur in listed:
                if cur >= len(ids):
                    raise IndexError("transformIncrements.at")
                plan[idx] = cur
                break
            if cur == parents[cur]:
                raise RuntimeError("Stuck in a loop, this should not happen")
    return plan


def mul44(A, B):
    """((a0 b0 + a1 b1) + a2 b2) + a3 b3 per entry."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    C = np.empty((4, 4))
    for i in range(4):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return C


def rigid_inverse(T):
    T = np.asarray(T, np.float64)
    O = np.eye(4)
    O[:3, :3] = T[:3, :3].T
    for i in range(3):
        O[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return O


def mapper_initial_guess(prev, odom_prev, odom_now, calib):
    """Mapper.cpp:250-260 with rigid inverses."""
    ci = rigid_inverse(calib)
    a, b = mul44(odom_now, ci), mul44(odom_prev, ci)
    return mul44(prev, mul44(rigid_inverse(b), a))


# ---- PlaceRecognition::getLoopClosureCandidatesIdxs (PlaceRecognition.cpp:231-284) ------------------------------------------
def loop_closure_candidates(col, lastFinishedSubmapIdx):
    p, adj = col.p, col.adjacencyMatrix_
    idxs = []
    lastCenter = col.submaps_[lastFinishedSubmapIdx].getMapToSubmapCenter()
    for i in range(len(col.submaps_)):
        if i == col.activeSubmapIdx_:
            continue
        if adj.isAdjacent(col.submaps_[i].id_, col.submaps_[col.activeSubmapIdx_].id_):
            continue
        if abs(i - lastFinishedSubmapIdx) == 1 or adj.isAdjacent(i, lastFinishedSubmapIdx):
            continue
        maxDistance = p["loop_closure_search_radius"]
        if norm3(lastCenter, col.submaps_[i].getMapToSubmapCenter()) > maxDistance:
            continue
        if abs(i - lastFinishedSubmapIdx) <= int(math.ceil(maxDistance / p["radius"])):
            continue
        if adj.getDistanceToNearestLoopClosureSubmap(lastFinishedSubmapIdx) < p["min_submaps_between_loop_closures"]:
            continue
        idxs.append(i)
    return idxs


# ---- computeOdometryConstraints, the pair selection (constraint_builders.cpp:92-118) ----------------------------------------
def odometry_constraint_pairs(col, candidates=None, existing=()):
    pairs = [tuple(e) for e in existing]
    out = []
    active = col.submaps_[col.activeSubmapIdx_].id_
    if candidates is not None:
        for c in candidates:
            if c < 1:
                continue
            src = col.submaps_[c].parentId_
            if (src, c) not in pairs:
                pairs.append((src, c))
                out.append((src, c))
    else:
        for tgt in range(1, len(col.submaps_)):
            src = col.submaps_[tgt].parentId_
            if (src, tgt) not in pairs and src != active and tgt != active:
                pairs.append((src, tgt))
                out.append((src, tgt))
    return out
